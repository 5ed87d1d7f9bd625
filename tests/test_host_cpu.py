"""CPU-only tests of the host side: C-ABI library loads and exports every symbol include/clamd.h declares, the
drop-in module surface matches the reference's state_dict, synthetic data is deterministic, engine geometry and
packing tables are consistent.  No kernel is launched here (there is no GPU in the build container)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def C():
    import continual_learning_amd as C
    return C


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(clamd_[a-z0-9_A-Z]+)\s*\(', src)))


def test_abi_library_exports_every_declared_symbol(C):
    names = header_functions()
    assert len(names) >= 25
    lib = ctypes.CDLL(C._lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/clamd.h but not exported by libclamd.so'
    assert sorted(C._lib.SIGNATURES) == names, 'ctypes signature table and header disagree'
    l = C._lib.load()
    assert l.clamd_version() >= 100
    assert l.clamd_sizeof_pack_job() == 136 and l.clamd_sizeof_adam_tensor() == 48
    assert l.clamd_bn_bwd_nsums() == 5
    assert l.clamd_sizeof_tuning() == ctypes.sizeof(C._lib.Tuning)


def test_header_prototypes_match_ctypes_signature_table(C):
    """Every prototype of include/clamd.h is parsed and compared, argument by argument, with _lib.SIGNATURES (pointer /
    int / double / long long / size_t classes): a stale binding would put an int into a pointer slot.
    INTEGRATION.md's example bindings are generated from the same table and checked here too."""
    src = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'typedef struct clamd_tuning \{.*?\} clamd_tuning;', '', src, flags=re.S)
    protos = re.findall(r'(?:^|\n)\s*((?:const\s+)?[a-z_ ]+?\**)\s*(clamd_[A-Za-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src)
    assert len(protos) == len(C._lib.SIGNATURES), (len(protos), len(C._lib.SIGNATURES))

    def klass(ctype):
        ctype = ctype.strip()
        if ctype in ('void', ''):
            return None
        if '*' in ctype:
            return 'char*' if ctype.replace('const', '').strip().startswith('char') else 'ptr'
        return {'int': 'int', 'double': 'double', 'long long': 'll', 'size_t': 'size', 'unsigned int': 'int'}[ctype.replace('const', '').strip()]

    from ctypes import c_char_p, c_double, c_int, c_longlong, c_size_t, c_void_p
    cls = {c_void_p: 'ptr', c_int: 'int', c_double: 'double', c_longlong: 'll', c_size_t: 'size', c_char_p: 'char*', None: None}
    for ret, name, args in protos:
        res, argtypes = C._lib.SIGNATURES[name]
        assert cls[res] == klass(ret), (name, ret)
        want = []
        for a in [a for a in args.split(',') if a.strip() and a.strip() != 'void']:
            a = a.strip()
            want.append(klass(a if a.endswith('*') else a.rsplit(' ', 1)[0] + ('*' if a.rsplit(' ', 1)[1].startswith('*') else '')))
        assert [cls[t] for t in argtypes] == want, f'{name}: header {want} vs ctypes {[cls[t] for t in argtypes]}'
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in re.findall(r"lib\.(clamd_[a-z0-9_]+)\.argtypes = \[([^\]]*)\]", doc):
        fn, listed = name
        short = {'ptr': 'P', 'int': 'I', 'double': 'D', 'll': 'LL', 'size': 'SZ', 'char*': 'S'}
        assert [x.strip() for x in listed.split(',')] == [short[cls[t]] for t in C._lib.SIGNATURES[fn][1]], f'INTEGRATION.md: stale argtypes for {fn}'


def test_stat_rows_and_tuning_are_per_call(C):
    """clamd_stat_rows answers from the same plan the launchers use; tuning arrives per call (no process state)."""
    L = C._lib
    lib = L.load()
    t = L.Tuning()
    assert t.as_dict()['igemm_pws'] == 1 and t.as_dict()['wgrad_blocks'] == 512 and t.cu_reserve == 0
    # persistent kernel: one row per workgroup of a 64-channel slab (256 CUs / slabs); producer/consumer kernel: one per tile
    assert L.stat_rows(L.OP_CONV3X3, 16, 256, 256, 64, 64, L.BF16) == 256
    assert L.stat_rows(L.OP_CONV3X3, 16, 256, 256, 64, 64, L.BF16, tuning=L.Tuning(cu_reserve=16)) == 240
    assert L.stat_rows(L.OP_CONV3X3, 16, 128, 128, 128, 128, L.BF16) == 128
    assert L.stat_rows(L.OP_CONV3X3, 16, 256, 256, 64, 64, L.BF16, tuning=L.Tuning(igemm_pws=0, igemm_ws=1)) == 16 * 32 * 8
    assert L.stat_rows(L.OP_CONV3X3, 16, 256, 256, 64, 64, L.F32, fused_bn=True) == 16 * 32 * 8     # pws declines fp32 + fused sums
    # Winograd kernels: one row per workgroup of the persistent grid, one per pixel tile when every tile has its own workgroup
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD, 16, 256, 256, 64, 64, L.F32) == 256
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD, 16, 256, 256, 64, 64, L.F32, tuning=L.Tuning(wino_persist=0)) == 16 * 16 * 16
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD24, 16, 256, 256, 64, 64, L.F32, tuning=L.Tuning(cu_reserve=8)) == 248
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD24, 16, 256, 256, 64, 64, L.F32, tuning=L.Tuning(wino_persist=0)) == 16 * 32 * 8
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD24, 1, 16, 16, 64, 64, L.F32) == 1                       # fewer tiles than CUs
    assert L.stat_rows(L.OP_CONV1X1, 2, 64, 64, 32, 64, L.F32) == 2 * 8 * 2
    # F(4x4): 32 tile blocks of 16 x 32 pixels here, 4 slabs; the half-width F(2x4) launch: 32-channel slabs, two workgroups per CU
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD44, 16, 64, 64, 256, 256, L.F32) == 256
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD44, 16, 64, 64, 256, 256, L.F32, tuning=L.Tuning(wino_persist=0)) == 16 * 4 * 2
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD44, 16, 64, 64, 256, 256, L.F32, tuning=L.Tuning(cu_reserve=8)) == 248
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD44, 1, 16, 32, 64, 64, L.F32) == 1
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD24, 16, 256, 256, 64, 64, L.F32, tuning=L.Tuning(wino_half=1)) == 512
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD24, 16, 256, 256, 64, 64, L.F32, tuning=L.Tuning(wino_half=1, cu_reserve=8)) == 496
    assert L.stat_rows(L.OP_CONV3X3_WINOGRAD24, 16, 256, 256, 64, 64, L.F32, tuning=L.Tuning(wino_half=1, wino_persist=0)) == 16 * 32 * 8
    assert L.stat_rows(L.OP_BN_BWD_REDUCE, 16, 256, 256, 0, 64, L.BF16) == 1024
    assert L.stat_rows(L.OP_BN_BWD_REDUCE, 16, 16, 16, 0, 1024, L.BF16) == 256
    assert lib.clamd_stat_rows(99, 1, 8, 8, 32, 32, 0, 0, None) < 0 and 'unknown op' in lib.clamd_last_error().decode()
    bad = L.Tuning(); bad.wgrad_blocks = 100000
    assert lib.clamd_stat_rows(L.OP_CONV3X3, 1, 8, 8, 32, 32, 0, 0, bad.ref()) < 0 and 'wgrad_blocks' in lib.clamd_last_error().decode()
    with pytest.raises(KeyError):
        L.Tuning(no_such_knob=1)
    m = C.UNet(2, 3, 4)
    m.tuning.wino_persist = 0
    assert C.UNet(2, 3, 4).tuning.wino_persist == 1          # per model, not per process


def test_winograd_size_queries_are_pinned(C):
    """The buffer-size queries of the Winograd entry points (pure host functions; values of the 256-CU plan, recorded before the launch
    layer was shared).  Shapes: W >= 32 and W < 32, exact and ragged tiles; channel counts 128 / 384 (the wave-level plan) and 256 / 512
    (workgroup blocks: the split-K bound answers except at 16 x 16, where the stream-K slots are larger); zero for empty or too-narrow
    arguments."""
    lib = C._lib.load()
    shapes = [(2, 64, 64), (16, 32, 32), (1, 16, 16), (3, 20, 36), (2, 24, 20), (16, 64, 64)]
    chans = ((128, 128), (256, 256), (384, 256), (512, 512), (256, 512), (512, 384))
    want = {
        '24': ([196608, 393216, 1572864, 393216, 786432, 3145728, 6144, 12288, 49152, 110592, 221184, 884736, 49152, 98304, 393216, 1572864,
                3145728, 12582912],
               [98304, 3145728, 196608, 6291456, 3072, 98304, 55296, 1769472, 24576, 786432, 786432, 25165824],
               [53477376, 201326592, 94371840, 201326592, 201326592, 113246208, 70778880, 201326592, 94371840, 201326592, 201326592, 113246208,
                6291456, 18874368, 37748736, 75497472, 37748736, 75497472, 59768832, 201326592, 75497472, 201326592, 201326592, 113246208,
                28311552, 100663296, 75497472, 201326592, 201326592, 113246208, 70778880, 201326592, 94371840, 201326592, 201326592, 113246208]),
        '44': ([147456, 294912, 1179648, 294912, 589824, 2359296, 9216, 18432, 73728, 110592, 221184, 884736, 36864, 73728, 294912, 1179648,
                2359296, 9437184],
               [73728, 2359296, 147456, 4718592, 4608, 147456, 55296, 1769472, 18432, 589824, 589824, 18874368],
               [42467328, 198180864, 99090432, 188743680, 188743680, 141557760, 56623104, 198180864, 99090432, 188743680, 188743680, 141557760,
                9437184, 28311552, 56623104, 75497472, 56623104, 113246208, 61341696, 198180864, 84934656, 188743680, 188743680, 141557760,
                23592960, 75497472, 84934656, 188743680, 150994944, 113246208, 73138176, 198180864, 99090432, 188743680, 188743680, 141557760]),
    }
    for form, (inp, opd, ws) in want.items():
        elems = getattr(lib, f'clamd_winograd{form}_input_elems')
        operand = getattr(lib, f'clamd_wgrad_winograd{form}_pre_operand_elems')
        wsb = getattr(lib, f'clamd_wgrad_winograd{form}_pre_workspace_bytes')
        assert [elems(*s, c) for s in shapes for c in (8, 20, 64)] == inp, form
        assert [operand(*s, c) for s in shapes for c in (4, 128)] == opd, form
        assert [wsb(*s, rp, cp) for s in shapes for rp, cp in chans] == ws, form
        assert [elems(*a) for a in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0))] == [0] * 4
        assert [operand(*a) for a in ((0, 8, 8, 8), (1, 8, 8, 0))] == [0] * 2
        assert [wsb(*a) for a in ((0, 32, 32, 256, 256), (1, 32, 32, 64, 256), (1, 32, 32, 256, 127), (1, 32, 0, 256, 256))] == [0] * 4
    # the in-kernel-transform weight gradients: slabs of 16 (F(2x2)) or 4 x 8 (F(2x4)) floats per channel pair, at most 512 workgroups of
    # 64 x 64 or 64 x 32 channels
    rc = [(r, c) for r in (32, 64, 96, 128, 256, 384, 512, 1024) for c in (32, 128, 384, 2048)]
    assert [lib.clamd_wgrad_winograd_workspace_bytes(r, c) for r, c in rc] == [
        33554432, 67108864, 66846720, 67108864, 67108864, 134217728, 133693440, 134217728, 50331648, 100663296, 99090432, 100663296,
        67108864, 134217728, 132120576, 134217728, 67108864, 134217728, 132120576, 134217728, 66846720, 132120576, 132120576, 100663296,
        67108864, 134217728, 125829120, 134217728, 67108864, 134217728, 125829120, 134217728]
    assert [lib.clamd_wgrad_winograd24_workspace_bytes(r, c) for r, c in rc] == [
        67108864, 67108864, 66060288, 67108864, 134217728, 134217728, 132120576, 134217728, 100663296, 100663296, 99090432, 100663296,
        134217728, 134217728, 132120576, 134217728, 134217728, 134217728, 125829120, 134217728, 133693440, 132120576, 132120576, 100663296,
        134217728, 134217728, 125829120, 134217728, 134217728, 134217728, 100663296, 268435456]


def test_module_surface_matches_reference_state_dict(C, golden):
    g = golden('unet_cd8_c21_64.npz')
    m = C.UNet(21, 3, 8)
    assert [n for n, _ in m.named_parameters()] == list(g['grad_names'])
    sd = m.state_dict()
    assert len(sd) == 136
    assert sd['dec1.block.6.weight'].shape == (128, 64, 2, 2)         # ConvTranspose2d [Cin, Cout, 2, 2]
    assert sd['enc2.block.1.weight'].shape == (16, 8, 3, 3)
    assert sd['last.6.weight'].shape == (21, 8, 1, 1)
    assert sd['enc1.2.num_batches_tracked'].dtype == torch.int64
    full = C.UNet(21)
    assert sum(p.numel() for p in full.parameters()) == 31_044_821
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 32, 32))                                    # no CPU fallback


def test_synth_is_deterministic_and_blocky(C):
    a = C.synth.images(1234, 2, 3, 32, 32)
    b = C.synth.images(1234, 4, 3, 32, 32)
    assert a.dtype == np.float32 and a.min() >= -1 and a.max() < 1
    assert np.array_equal(a, b[:2])
    assert np.array_equal(C.synth.images(1234, 2, 3, 32, 32, first_image=2), b[2:])
    l = C.synth.labels(1234, 2, 64, 64, 21)
    assert l.dtype == np.int64 and l.min() >= 0 and l.max() < 21
    assert (l[:, :16, :16] == l[:, :1, :1]).all()
    l2 = C.synth.labels(1234, 2, 64, 64, 21, class_lo=11, class_hi=21)
    assert set(np.unique(l2)) <= {0, *range(11, 21)}
    w = C.synth.closed_form_tensor('enc1.0.weight', (4, 3, 3, 3))
    assert np.abs(w).max() <= 1 / np.sqrt(27) + 1e-7


def test_engine_geometry_and_pack_table(C):
    from continual_learning_amd.unet import _Engine, _FoldSource
    m = C.UNet(21, 3, 8)
    e = _Engine(m, 2, 64, 64, torch.device('cpu'))
    assert len(e.convs) == 18 and len(e.stages) == 9
    assert e.gflat.numel() == sum(p.numel() for p in m.parameters())
    # flat gradient buffer is in reverse registration order: the head's bias first, enc1.0.weight last
    assert e.goffset['last.6.bias'][0] == 0
    assert e.goffset['enc1.0.weight'][0] + e.goffset['enc1.0.weight'][1] == e.gflat.numel()
    dec2a = [u for u in e.convs if u.name == 'dec2.block.0'][0]
    assert dec2a.cin_segs == [(64, 64), (64, 64)] and dec2a.xin is e.cat[3]
    enc1b = [u for u in e.convs if u.name == 'enc1.3'][0]
    assert enc1b.out is e.cat[0] and enc1b.pooled is e.pool[0] and enc1b.out_ldc == 64
    jobs = e.pack_table.jobs + e.pack_late.jobs           # two launches: what enc1-enc3 need first, the rest on the second stream
    assert not any(u.pack_late for u in e.convs[:6]) and all(u.pack_late for u in e.convs[6:])
    # wf + wd + bias per conv (no wd for enc1.0), 3 per tail; on the fp32 path the filters of the Winograd units
    # (3x3, even images of at least 8x8: every unit here except enc1.0 (im2col) and the two 4x4 centre convs) are
    # transformed by the Winograd pack table instead
    wino = lambda u: u.plan.fwd not in ('im2col', 'igemm')    # the unit's forward runs a Winograd form (plan.ALGOS)
    wino_units = [u for u in e.convs if wino(u)]
    assert len(wino_units) == 15 and all(min(u.h, u.width) >= 8 for u in wino_units)
    w24 = [u for u in wino_units if u.plan.fwd != 'f22']
    assert len(w24) == 15                                   # every width here (64 ... 8) is a multiple of 4: F(2x4,3x3)
    nw = sum(len(t.jobs) for t in e.wino_early + e.wino_late)          # two launches per form: enc1-enc3 first, the rest behind
    # the second convolution of every block here (<= 128 channels) is a candidate for the algebraic BatchNorm fold (bnfold.hip): its
    # forward filters are packed inside the step by a one-job table of its own (with the producer's scale, or plain)
    fold = [u for u in e.convs if u.fold_a is not None]
    # ... plus the two readers of enc3's output (32 channels = its padded count; 64 x 64 input: 16 x 16 there), whose BatchNorm is folded
    # into both: the block's second conv writes its conv+ReLU output into the concat buffer and only a pooling pass is left
    pooled = [u for u in e.convs if u.pool_fold]
    assert [u.name for u in pooled] == ['enc3.block.4'] and pooled[0].y is e.cat[2] and pooled[0].y_ldc == 64
    assert sorted(u.name for u in fold if isinstance(u.fold_a, _FoldSource)) == ['dec3.block.0', 'enc4.block.1']
    assert len(fold) == 11 and all(u.fold_a.apply_in_filters and len(u.fold_table.jobs) == 1 and len(u.plain_table.jobs) == 1 for u in fold)
    ks = lambda u, t: t.jobs[0][-1 if wino(u) else -2]       # kscale: the last field of a Winograd pack job, the one before dst_t of a plain one
    assert all(ks(u, u.fold_table) == u.fold_a.vec[0].data_ptr() and ks(u, u.plain_table) == 0 for u in fold)
    assert sum(len(t.jobs) for t in e.wino_early) == sum(2 - (u.fold_a is not None) for u in wino_units if not u.pack_late)
    assert nw == 2 * len(wino_units) - sum(1 for u in fold if wino(u))
    head = e.stages[-1]['tail']
    assert head.kind == 'head' and head.fold_b is e.convs[-1] and len(head.fold_table.jobs) == 1      # the 1x1 head folds the last BatchNorm
    # a plain (non-Winograd) 3x3 unit whose forward AND data-gradient filters come from the table is ONE job (PackJob::dst_t: both layouts from one
    # read of the source tile)
    merged = [j for j in jobs if j[2] == 9 and j[-1] != 0]
    assert len(merged) == sum(1 for u in e.convs if not wino(u) and u.plan.fwd != 'im2col' and u.fold_a is None and u.wd is not None)
    assert len(jobs) + len(merged) + nw + len(fold) + 1 == 18 * 3 - 1 + 5 * 3
    assert e.pack_table.nblocks + e.pack_late.nblocks == sum(((j[3] + 31) // 32) * ((j[4] + 31) // 32) for j in jobs)
    assert C.cpad(3) == 32 and C.cpad(21) == 32 and C.cpad(1024) == 1024


def test_fold_plan_at_the_reference_width(C):
    """Planning only (no kernel runs without a GPU): at conv_dim 64 the algebraic BatchNorm folds of bnfold.hip cover the second convolution of
    enc1 / enc2 / dec4 / last, the 1x1 head, and both readers of enc1's output (its conv+ReLU output lives in the concat buffer); the wide
    layers fold through their transform kernels instead; bf16 folds the same 3x3 pairs."""
    from continual_learning_amd.unet import _Engine, _FoldSource
    e = _Engine(C.UNet(21, 3, 64), 2, 64, 64, torch.device('cpu'))
    pair = sorted(u.name for u in e.convs if u.fold_a is not None and not isinstance(u.fold_a, _FoldSource))
    assert pair == ['dec4.block.3', 'enc1.3', 'enc2.block.4', 'last.3']
    assert [u.name for u in e.convs if u.pool_fold] == ['enc1.3']
    readers = {u.name: u.fold_a for u in e.convs if isinstance(u.fold_a, _FoldSource)}
    assert sorted(readers) == ['enc2.block.1', 'last.0']
    enc1b = next(u for u in e.convs if u.name == 'enc1.3')
    assert readers['last.0'].y is e.cat[0] and readers['enc2.block.1'].y is e.pool[0] and enc1b.y is e.cat[0] and enc1b.y_ldc == 128
    # the block's scale / shift vectors are the first halves of the decoder convolution's [scale | 1], [shift | 0]
    assert enc1b.vec[0].data_ptr() == readers['last.0'].vec[0].data_ptr() and enc1b.vec[1].data_ptr() == readers['last.0'].vec[1].data_ptr()
    assert torch.equal(readers['last.0'].vec[0][64:], torch.ones(64)) and torch.equal(readers['last.0'].vec[1], torch.zeros(128))
    # (64 x 64 input: 4 x 4 images at the bottom, where the Winograd kernels do not apply)
    assert sorted(u.name for u in e.convs if u.apply_folded) == ['dec2.block.0', 'dec3.block.0', 'enc3.block.1', 'enc4.block.1']
    assert e.stages[-1]['tail'].fold_b.name == 'last.3'
    eb = _Engine(C.UNet(21, 3, 64, compute_dtype='bf16'), 2, 64, 64, torch.device('cpu'))
    # bf16 (round 4: the fold pays there too, tools/step_ab.py bf16 FOLD_BN_INTO_FILTERS): the same four pairs; the pooled / skip readers of an
    # encoder block's output stay unfolded (that fold moves the raw tensor into the concat buffer, so it cannot depend on the tuning)
    assert sorted(u.name for u in eb.convs if u.fold_a is not None) == pair and not any(u.pool_fold for u in eb.convs)
    assert eb.stages[-1]['tail'].fold_b is not None


def test_fused_adam_state_dict_layout_without_gpu(C):
    p = torch.nn.Parameter(torch.zeros(3))
    opt = C.FusedAdam([p], lr=1e-4, betas=[0.5, 0.99])
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-4, betas=[0.5, 0.99])
    a, b = opt.state_dict()['param_groups'][0], ref.state_dict()['param_groups'][0]
    for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params'):
        assert a[k] == b[k] or list(a[k]) == list(b[k])
    p.grad = torch.zeros(3)
    with pytest.raises(RuntimeError):
        opt.step()                                     # CPU parameters: fails loudly


def test_crop_origin_matches_pad_center_crop(C):
    """Host geometry of the GPU data path vs the oracle's Pad(10)+CenterCrop restatement, incl. undersized images."""
    from oracle import np_unet as O
    rng = np.random.default_rng(0)
    for hs, ws, h, w in [(300, 500, 256, 256), (375, 500, 512, 256), (100, 90, 256, 256), (237, 333, 256, 256), (256, 256, 256, 256)]:
        a = rng.integers(1, 255, (hs, ws, 1)).astype(np.uint8)
        ref = O.pad_center_crop(a, h, w)[..., 0]
        oy, ox = C.data.crop_origin(hs, ws, h, w)
        ys, xs = np.arange(h) + oy, np.arange(w) + ox
        got = np.zeros((h, w), np.uint8)
        vy, vx = (ys >= 0) & (ys < hs), (xs >= 0) & (xs < ws)
        got[np.ix_(vy, vx)] = a[np.ix_(ys[vy], xs[vx])][..., 0]
        assert np.array_equal(got, ref), (hs, ws, h, w)


_CONV = 'x x_ldc w bias y y_ldc stats stat_rows B H W Cin_p Cout_p relu tune stream'.split()
_CONV_PRE = 'v w bias y y_ldc stats stat_rows B H W Cin_p Cout_p relu tune stream'.split()
_XFORM = 'x x_ldc scale shift v B H W Cp stream'.split()
_WGRAD = 'gz gz_ldc x x_ldc ws ws_bytes out B H W Rp Cp R C r_seg0 r_seg0p c_seg0 c_seg0p tune stream'.split()
_WGRAD_PRE = 'gz gz_ldc v yt ws ws_bytes out B H W Rp Cp R C r_seg0 r_seg0p c_seg0 c_seg0p tune stream'.split()
_YT = 'gz gz_ldc yt B H W Rp stream'.split()


def _refusal_tools(lib):
    def refused(name, order, base, want, **kw):
        a = dict(base)
        a.update(kw)
        rc = getattr(lib, name)(*[a[k] for k in order])
        msg = lib.clamd_last_error().decode()
        assert rc == -1 and msg == want, (name, kw, rc, msg, want)

    def chain(name, order, base, steps):
        """steps: (message, overrides) in the order of the checks; each alone, and each together with its successor"""
        for i, (want, kw) in enumerate(steps):
            refused(name, order, base, want, **kw)
            if i + 1 < len(steps):
                refused(name, order, base, want, **{**steps[i + 1][1], **kw})

    return refused, chain


def _check_winograd_refusals(lib, tref, bad_tune):
    """Every refusal branch of the launching Winograd entry points, with the WHOLE message (the entry point's prefix included) and
    status -1 (a host check; -2 would be a launch that was tried).  Consecutive branches are also violated together: the earlier check
    answers.  Nothing here passes validation, so no pointer is dereferenced."""
    p = 0x1000
    big = 1 << 30                                           # batch: 2^31 or more workgroups of any of the kernels at 32 x 32
    refused, chain = _refusal_tools(lib)

    tuning = ('tuning: wino_mt 0..2', dict(tune=bad_tune))
    rows = 'stat_rows does not match clamd_stat_rows(CLAMD_OP_CONV3X3_WINOGRAD%s, ...)'

    conv = dict(x=None, x_ldc=64, w=None, bias=None, y=None, y_ldc=64, stats=None, stat_rows=0, B=1, H=32, W=32, Cin_p=64, Cout_p=64, relu=0,
                tune=None, stream=None)
    n = 'conv3x3_winograd: '
    chain('clamd_conv3x3_winograd', _CONV, conv, [
        (n + 'empty problem', dict(B=0)),
        (n + 'H and W must be even (2x2 output tiles)', dict(H=15)),
        (n + 'channel counts/pitches must be padded', dict(Cin_p=40)),
        (n + 'image or filter exceeds 2^31 bytes', dict(H=4096, W=4096)),
        tuning,
        (n + 'relu must be 0 or 1 (no border-class bias here)', dict(relu=2)),
        (n + 'grid out of range', dict(B=big)),
        (n + rows % '', dict(stats=p, stat_rows=7))])
    refused('clamd_conv3x3_winograd', _CONV, conv, n + 'H and W must be even (2x2 output tiles)', W=31)
    for kw in (dict(Cout_p=48), dict(x_ldc=68), dict(y_ldc=4)):
        refused('clamd_conv3x3_winograd', _CONV, conv, n + 'channel counts/pitches must be padded', **kw)
    refused('clamd_conv3x3_winograd', _CONV, conv, n + 'image or filter exceeds 2^31 bytes', Cin_p=8192, Cout_p=8192, x_ldc=8192, y_ldc=8192)

    for half, n in ((0, 'conv3x3_winograd24: '), (1, 'conv3x3_winograd24 (half-width): ')):
        t = tref(wino_half=half)
        chain('clamd_conv3x3_winograd24', _CONV, dict(conv, tune=t), [
            ('conv3x3_winograd24: empty problem', dict(H=0)),
            ('conv3x3_winograd24: H must be even and W a multiple of 4 (2x4 output tiles)', dict(W=30)),
            ('conv3x3_winograd24: channel counts/pitches must be padded', dict(y_ldc=68)),
            ('conv3x3_winograd24: image or filter exceeds 2^31 bytes', dict(H=4096, W=4096)),
            tuning,
            ('conv3x3_winograd24: bad relu flags (bit 1 needs the [9][Cout_p] bias table)', dict(relu=4)),
            (n + 'grid out of range', dict(B=big)),
            (n + rows % '24', dict(stats=p, stat_rows=3))])
        refused('clamd_conv3x3_winograd24', _CONV, dict(conv, tune=t), 'conv3x3_winograd24: bad relu flags (bit 1 needs the [9][Cout_p] bias table)', relu=2)
        refused('clamd_conv3x3_winograd24', _CONV, dict(conv, tune=t), 'conv3x3_winograd24: H must be even and W a multiple of 4 (2x4 output tiles)', H=31)
    # the rows of a half-width launch differ from the full-width ones (512 against 256 here): each is refused with the other's count
    wide = dict(conv, B=16, H=256, W=256, stats=p)
    refused('clamd_conv3x3_winograd24', _CONV, wide, 'conv3x3_winograd24: ' + rows % '24', stat_rows=512)
    refused('clamd_conv3x3_winograd24', _CONV, wide, 'conv3x3_winograd24 (half-width): ' + rows % '24', stat_rows=256, tune=tref(wino_half=1))

    n = 'conv3x3_winograd24_direct_filters: '
    chain('clamd_conv3x3_winograd24_direct_filters', _CONV, conv, [
        (n + 'empty problem', dict(B=-1)),
        (n + 'H must be even and W a multiple of 4 (2x4 output tiles)', dict(W=34)),
        (n + 'needs Cin_p % 32 == 0, Cout_p % 64 == 0', dict(Cout_p=96)),
        (n + 'image or filter exceeds 2^31 bytes', dict(H=4096, W=4096)),
        tuning,
        (n + 'grid out of range', dict(B=big)),
        (n + rows % '24', dict(stats=p, stat_rows=3)),
        (n + 'bad relu flags (bit 1 needs the [9][Cout_p] bias table)', dict(relu=2))])
    refused('clamd_conv3x3_winograd24_direct_filters', _CONV, conv, n + 'needs Cin_p % 32 == 0, Cout_p % 64 == 0', Cin_p=48)
    refused('clamd_conv3x3_winograd24_direct_filters', _CONV, conv, n + 'bad relu flags (bit 1 needs the [9][Cout_p] bias table)', relu=5, bias=p)
    # its rows follow clamd_stat_rows(CLAMD_OP_CONV3X3_WINOGRAD24), which answers for the half-width launch under wino_half
    refused('clamd_conv3x3_winograd24_direct_filters', _CONV, wide, n + rows % '24', stat_rows=256, tune=tref(wino_half=1))

    xf = dict(x=None, x_ldc=64, scale=None, shift=None, v=None, B=1, H=32, W=32, Cp=64, stream=None)
    for form, even, hbad in (('24', 'H must be even and W a multiple of 4 (2x4 output tiles)', 31), ('44', 'H and W must be multiples of 4 (4x4 output tiles)', 30)):
        n = f'winograd{form}_transform_input: '
        chain(f'clamd_winograd{form}_transform_input', _XFORM, xf, [
            (n + 'scale and shift go together', dict(scale=p)),
            (n + 'empty problem', dict(B=0)),
            (n + even, dict(H=hbad)),
            (n + 'channel count / pitch must be padded', dict(Cp=12)),
            (n + 'image exceeds 2^31 bytes', dict(H=4096, W=4096, x_ldc=32, Cp=32)),
            (n + 'grid out of range', dict(B=2 * big - 1, H=64))])
        refused(f'clamd_winograd{form}_transform_input', _XFORM, xf, n + 'scale and shift go together', shift=p)
        refused(f'clamd_winograd{form}_transform_input', _XFORM, xf, n + even, W=34)
        for kw in (dict(x_ldc=66), dict(x_ldc=32)):
            refused(f'clamd_winograd{form}_transform_input', _XFORM, xf, n + 'channel count / pitch must be padded', **kw)
    # the F(4x4) transform runs two workgroups per tile block: 2^30 blocks are out of its range
    refused('clamd_winograd44_transform_input', _XFORM, xf, 'winograd44_transform_input: grid out of range', B=big, H=16, Cp=8, x_ldc=8)

    pre = dict(v=None, w=None, bias=None, y=None, y_ldc=64, stats=None, stat_rows=0, B=1, H=32, W=32, Cin_p=64, Cout_p=64, relu=0, tune=None, stream=None)
    for form, even, hbad, needs, chan in (
            ('24', 'H must be even and W a multiple of 4 (2x4 output tiles)', 31, 'needs Cin_p % 32 == 0, Cin_p >= 64, Cout_p % 64 == 0',
             (dict(Cin_p=32), dict(Cin_p=72), dict(Cout_p=96), dict(y_ldc=68))),
            ('44', 'H and W must be multiples of 4 (4x4 output tiles)', 30, 'needs Cin_p % 8 == 0, Cin_p >= 16, Cout_p % 64 == 0',
             (dict(Cin_p=8), dict(Cin_p=20), dict(Cout_p=96), dict(y_ldc=66)))):
        name, n = f'clamd_conv3x3_winograd{form}_pre', f'conv3x3_winograd{form}_pre: '
        chain(name, _CONV_PRE, pre, [
            (n + 'empty problem', dict(W=0)),
            (n + even, dict(H=hbad)),
            (n + needs, chan[0]),
            tuning,
            (n + 'grid out of range', dict(B=big)),
            (n + 'transformed input exceeds 2^32 bytes or filter 2^31 bytes', dict(B=128, H=256, W=256, Cin_p=128)),
            (n + rows % form, dict(stats=p, stat_rows=5)),
            (n + 'relu must be 0 or 1 (no border-class bias here)', dict(relu=2))])
        for kw in chan[1:]:
            refused(name, _CONV_PRE, pre, n + needs, **kw)
        refused(name, _CONV_PRE, pre, n + even, W=34)
        refused(name, _CONV_PRE, pre, n + 'transformed input exceeds 2^32 bytes or filter 2^31 bytes', Cin_p=8192, Cout_p=8192)
    refused('clamd_conv3x3_winograd24_pre', _CONV_PRE, dict(pre, B=16, H=256, W=256, stats=p), 'conv3x3_winograd24_pre: ' + rows % '24', stat_rows=256,
            tune=tref(wino_half=1))
    # F(4x4) alone bounds the output image, after every other check
    n = 'conv3x3_winograd44_pre: '
    refused('clamd_conv3x3_winograd44_pre', _CONV_PRE, pre, n + 'one output image exceeds 2^31 bytes', H=4096, W=4096, Cin_p=16)
    refused('clamd_conv3x3_winograd44_pre', _CONV_PRE, pre, n + 'relu must be 0 or 1 (no border-class bias here)', H=4096, W=4096, Cin_p=16, relu=3)

    wg = dict(gz=None, gz_ldc=64, x=None, x_ldc=64, ws=None, ws_bytes=0, out=None, B=1, H=32, W=32, Rp=64, Cp=64, R=64, C=64, r_seg0=64, r_seg0p=64,
              c_seg0=64, c_seg0p=64, tune=None, stream=None)
    for form, even, wbad in (('', 'H and W must be even', 31), ('24', 'H must be even and W a multiple of 4', 30)):
        name, n = f'clamd_wgrad_winograd{form}', f'wgrad_winograd{form}: '
        chain(name, _WGRAD, wg, [
            tuning,
            (n + 'empty problem', dict(B=0)),
            (n + even, dict(W=wbad)),
            (n + 'channel counts/pitches must be padded', dict(Rp=48)),
            (n + 'one image exceeds 2^30 bytes', dict(H=2048, W=2048)),
            (n + 'workspace too small', dict(ws_bytes=16 * 64 * 64 * 4 - 1))])
        refused(name, _WGRAD, wg, n + even, H=31)
        for kw in (dict(Cp=40), dict(gz_ldc=68), dict(x_ldc=68)):
            refused(name, _WGRAD, wg, n + 'channel counts/pitches must be padded', **kw)
        refused(name, _WGRAD, wg, n + 'one image exceeds 2^30 bytes', H=2048, W=2048, gz_ldc=32)

    wp = dict(gz=None, gz_ldc=256, v=None, yt=None, ws=None, ws_bytes=0, out=None, B=1, H=32, W=32, Rp=256, Cp=256, R=256, C=256, r_seg0=256,
              r_seg0p=256, c_seg0=256, c_seg0p=256, tune=None, stream=None)
    for form, planes, even, hbad in (('24', 24, 'H must be even and W a multiple of 4', 31), ('44', 36, 'H and W must be multiples of 4', 30)):
        name, n = f'clamd_wgrad_winograd{form}_pre', f'wgrad_winograd{form}_pre: '
        chain(name, _WGRAD_PRE, wp, [
            tuning,
            (n + 'empty problem', dict(H=0)),
            (n + even, dict(H=hbad)),
            (n + 'needs Rp and Cp multiples of 128', dict(Rp=192)),
            (n + 'one image exceeds 2^31 bytes', dict(gz=p, H=4096, W=4096)),
            (n + 'an operand exceeds 2^32 bytes', dict(B=1024, H=256, W=256)),
            (n + 'workspace too small', dict(ws_bytes=planes * 256 * 256 * 4 - 1))])
        refused(name, _WGRAD_PRE, wp, n + even, W=34)
        for kw in (dict(Cp=64), dict(Rp=0), dict(Cp=-128), dict(gz_ldc=258)):
            refused(name, _WGRAD_PRE, wp, n + 'needs Rp and Cp multiples of 128', **kw)
        refused(name, _WGRAD_PRE, wp, n + 'an operand exceeds 2^32 bytes', B=256, H=256, W=256, Cp=2048)
        refused(name, _WGRAD_PRE, wp, n + 'workspace too small', tune=tref(wgrad_streamk=0), Rp=512, Cp=512)
        # the stream-K plans (gz == NULL: nothing runs before them) size their own slots; both forms share those launchers and their messages
        sk = 'wgrad_winograd_pre: workspace too small'
        refused(name, _WGRAD_PRE, wp, sk, Rp=128)                                            # wave-level plan
        refused(name, _WGRAD_PRE, wp, sk, Cp=384, tune=tref(wgrad_streamk=0))
        refused(name, _WGRAD_PRE, wp, sk, tune=tref(wgrad_streamk=2))
        refused(name, _WGRAD_PRE, wp, sk, Rp=512, Cp=512)                                    # planes x 4 items x 8 >= 3 x 256 CUs: stream-K by default
    # 24 x 2 x 8 = 384 < 768 <= 36 x 3 x 8: the same channel counts choose split-K in F(2x4) and stream-K in F(4x4)
    refused('clamd_wgrad_winograd24_pre', _WGRAD_PRE, wp, 'wgrad_winograd24_pre: workspace too small', Rp=512)
    refused('clamd_wgrad_winograd44_pre', _WGRAD_PRE, wp, 'wgrad_winograd_pre: workspace too small', Rp=768)
    refused('clamd_wgrad_winograd44_pre', _WGRAD_PRE, wp, 'wgrad_winograd44_pre: workspace too small', Rp=512)

    yt = dict(gz=p, gz_ldc=64, yt=p, B=1, H=32, W=32, Rp=64, stream=None)
    for form, even, hbad in (('24', 'H must be even and W a multiple of 4', 31), ('44', 'H and W must be multiples of 4', 30)):
        name, n = f'clamd_wgrad_winograd{form}_pre_transform', f'wgrad_winograd{form}_pre_transform: '
        chain(name, _YT, yt, [
            (n + 'bad arguments', dict(gz=None)),
            (n + even, dict(H=hbad)),
            (n + 'channel count / pitch must be padded', dict(Rp=6)),
            (n + 'operand too large', dict(H=4096, W=4096, gz_ldc=32))])
        for kw in (dict(yt=None), dict(B=0), dict(W=-4)):
            refused(name, _YT, yt, n + 'bad arguments', **kw)
        refused(name, _YT, yt, n + even, W=34)
        for kw in (dict(Rp=0), dict(gz_ldc=66)):
            refused(name, _YT, yt, n + 'channel count / pitch must be padded', **kw)
        refused(name, _YT, yt, n + 'operand too large', B=2048, H=256, W=256, Rp=128)

    for form in ('', '24', '44'):
        for args in ((None, 0, 0, None), (p, 1, 0, None), (p, 0, 4, None)):
            assert getattr(lib, f'clamd_wino{form}_pack')(*args) == -1 and lib.clamd_last_error().decode() == f'wino{form}_pack: empty job table'


_C3 = 'x x_ldc w bias y y_ldc stats bn_y bn_sums stat_rows B H W Cin_p Cout_p relu m_fastest dtype tune stream'.split()
_C1 = 'x x_ldc w bias y y_ldc stats bn_y bn_sums stat_rows B H W Cin_p Cout_p relu dtype stream'.split()
_LOGITS = 'x x_ldc w bias logits B H W Cin_p Cout_p num_classes dtype stream'.split()
_ARGMAX = 'x x_ldc w bias pred logits B H W Cin_p Cout_p num_classes dtype stream'.split()
_CT_FWD = 'x x_ldc w bias y y_ldc B H W Cin_p Cout_p dtype stream'.split()
_CT_DGRAD = 'gy gy_ldc w gx gx_ldc bn_y bn_sums stat_rows B H W Cin_p Cout_p dtype stream'.split()
_WG = 'mode a a_ldc b b_ldc ws ws_bytes out B H W Rp Cp R C r_seg0 r_seg0p c_seg0 c_seg0p dtype tune stream'.split()
_ROWS = 'op B H W Cin_p Cout_p dtype fused_bn tune'.split()


def _check_direct_conv_refusals(lib, tref, bad_tune, ops):
    """Every refusal of the direct-convolution, pointwise / ConvTranspose2d GEMM and weight-gradient entry points (igemm*.hip, wgrad*.hip)
    and of clamd_stat_rows, with the WHOLE message and status -1; consecutive checks are also violated together and the earlier one
    answers.  Nothing here passes validation: no pointer is dereferenced and nothing is launched."""
    p, odd = 0x1000, 0x1010                                 # 64-byte aligned / not
    big = 1 << 30
    refused, chain = _refusal_tools(lib)
    F32, SPLIT, NODT = 0, 2, 9
    split = 'bf16x3 tensors need a 64-byte aligned base and a pitch that is a multiple of 16 channels'
    padded = 'igemm: channel counts/pitches must be padded (K,N %32, ldc %8)'
    image, out_image, filt = 'igemm: one image exceeds 2^31 bytes', 'igemm: one output image exceeds 2^31 bytes', 'igemm: packed filter exceeds 2^31 bytes'
    tuning = ('tuning: wino_mt 0..2', dict(tune=bad_tune))
    rows = '%s: stat_rows = %d but this launch writes %d partial rows (size the buffer with clamd_stat_rows)'
    # the checks every GEMM entry point shares, in their order (x / y stand for the entry point's input / output argument names)
    common = lambda x, y, cin: [
        ('igemm: empty problem', dict(B=0)),
        (split, {'dtype': SPLIT, x: odd}),
        (padded, {cin: 40}),
        (image, {'H': 4096, 'W': 4096, x + '_ldc': 64, y + '_ldc': 8}),
        (out_image, {'H': 4096, 'W': 4096, x + '_ldc': 8, y + '_ldc': 64}),
        (filt, dict(Cin_p=8192, Cout_p=8192))]

    c3 = dict(x=None, x_ldc=64, w=None, bias=None, y=None, y_ldc=64, stats=None, bn_y=None, bn_sums=None, stat_rows=0, B=1, H=32, W=32, Cin_p=64,
              Cout_p=64, relu=0, m_fastest=0, dtype=F32, tune=None, stream=None)
    n = 'conv3x3: '
    direct, ws1 = tref(igemm_pws=0, igemm_ws=0), tref(igemm_pws=0, igemm_ws=1)
    chain('clamd_conv3x3', _C3, c3, [
        (n + 'bad relu flags', dict(relu=4))] + common('x', 'y', 'Cin_p') + [
        tuning,
        (n + 'bn_y and bn_sums go together', dict(bn_y=p)),
        (n + 'grid out of range', dict(B=big, tune=direct)),
        (n + 'the border-class bias table needs the persistent kernel (ask clamd_conv3x3_border_bias_ok), a table and H, W >= 2', dict(relu=2)),
        (rows % ('conv3x3', 7, 4), dict(stats=p, stat_rows=7)),
        ('igemm_pws: bad dtype', dict(dtype=NODT)),
        ('igemm_pws: grid out of range', dict(B=big))])
    for kw in (dict(y=odd), dict(bn_y=odd, bn_sums=p), dict(x=p, x_ldc=72), dict(y=p, y_ldc=72), dict(bn_y=p, bn_sums=p, Cout_p=72)):
        refused('clamd_conv3x3', _C3, c3, split, dtype=SPLIT, **kw)
    for kw in (dict(Cout_p=48), dict(x_ldc=68), dict(y_ldc=68)):
        refused('clamd_conv3x3', _C3, c3, padded, **kw)
    refused('clamd_conv3x3', _C3, c3, n + 'bn_y and bn_sums go together', bn_sums=p, stat_rows=4)
    refused('clamd_conv3x3', _C3, c3, n + 'grid out of range', B=big, tune=ws1)
    bias_table = n + 'the border-class bias table needs the persistent kernel (ask clamd_conv3x3_border_bias_ok), a table and H, W >= 2'
    for kw in (dict(bias=p, tune=direct), dict(bias=p, tune=ws1), dict(bias=p, H=1), dict(bias=p, W=1), dict(bias=p, Cin_p=512)):
        refused('clamd_conv3x3', _C3, c3, bias_table, relu=3, **kw)
    # the rows are those of the structure the plan chose: workgroups of the persistent kernel, 256- / 512- / 128-pixel tiles
    for t, have in ((direct, 4), (ws1, 4), (tref(igemm_pws=0, igemm_ws=3), 2), (tref(igemm_pws=0, igemm_ws=4), 8)):
        refused('clamd_conv3x3', _C3, c3, rows % ('conv3x3', 7, have), stats=p, stat_rows=7, tune=t)
    refused('clamd_conv3x3', _C3, c3, rows % ('conv3x3', 3, 4), bn_y=p, bn_sums=p, stat_rows=3)
    # each structure's launcher answers for the dtype first, then for its own grid (2^32 workgroups: 2^30 tiles x 4 slabs)
    for t, who in ((direct, 'igemm'), (ws1, 'igemm_ws')):
        refused('clamd_conv3x3', _C3, c3, who + ': bad dtype', dtype=NODT, tune=t)
        refused('clamd_conv3x3', _C3, c3, who + ': bad dtype', dtype=NODT, tune=t, B=big >> 2, Cout_p=256)
        refused('clamd_conv3x3', _C3, c3, who + ': grid out of range', tune=t, B=big >> 2, Cout_p=256)

    c1 = {k: v for k, v in c3.items() if k not in ('m_fastest', 'tune')}
    n = 'conv1x1: '
    chain('clamd_conv1x1', _C1, c1, [
        (n + 'relu must be 0 or 1', dict(relu=2))] + common('x', 'y', 'Cin_p') + [
        (n + 'bn_y and bn_sums go together', dict(bn_y=p)),
        (rows % ('conv1x1', 7, 4), dict(stats=p, stat_rows=7)),
        ('igemm: bad dtype', dict(dtype=NODT)),
        ('igemm: grid out of range', dict(B=big >> 2, Cout_p=256))])
    refused('clamd_conv1x1', _C1, c1, n + 'bn_y and bn_sums go together', bn_sums=p, stat_rows=4)
    refused('clamd_conv1x1', _C1, c1, rows % ('conv1x1', 3, 8), bn_y=p, bn_sums=p, stat_rows=3, B=2, H=17, W=18)
    refused('clamd_conv1x1', _C1, c1, split, dtype=SPLIT, bn_y=odd, bn_sums=p)

    lg = dict(x=None, x_ldc=64, w=None, bias=None, logits=None, pred=p, B=1, H=32, W=32, Cin_p=64, Cout_p=64, num_classes=21, dtype=F32, stream=None)
    head = lambda: [                         # the fp32 NCHW output is no NHWC tensor: no bf16x3 check of it, and its pitch stands in as 8
        ('igemm: empty problem', dict(W=0)),
        (split, dict(dtype=SPLIT, x=odd)),
        (padded, dict(Cin_p=40)),
        (image, dict(H=4096, W=4096)),
        (filt, dict(Cin_p=8192, Cout_p=8192))]
    chain('clamd_conv1x1_logits', _LOGITS, lg, head() + [
        ('conv1x1_logits: num_classes > padded Cout', dict(num_classes=65)),
        ('igemm: bad dtype', dict(dtype=NODT)),
        ('igemm: grid out of range', dict(B=big >> 2, Cout_p=256))])
    refused('clamd_conv1x1_logits', _LOGITS, lg, 'conv1x1_logits: num_classes > padded Cout', dtype=SPLIT, logits=odd, num_classes=65)
    n = 'conv1x1_argmax: '
    chain('clamd_conv1x1_argmax', _ARGMAX, lg, head() + [
        (n + 'pred is null', dict(pred=None)),
        (n + 'num_classes must be in [1, min(64, padded Cout)]', dict(num_classes=0)),
        (n + 'padded Cout must be 32 or 64 (the arg-max runs inside one 64-channel slab)', dict(Cout_p=96)),
        ('igemm: bad dtype', dict(dtype=NODT))])
    for kw in (dict(num_classes=65, Cout_p=96), dict(num_classes=33, Cout_p=32)):
        refused('clamd_conv1x1_argmax', _ARGMAX, lg, n + 'num_classes must be in [1, min(64, padded Cout)]', **kw)

    ct = dict(x=None, x_ldc=64, w=None, bias=None, y=None, y_ldc=64, B=1, H=32, W=32, Cin_p=64, Cout_p=64, dtype=F32, stream=None)
    chain('clamd_convT2x2_fwd', _CT_FWD, ct, common('x', 'y', 'Cin_p')[:5] + [
        (filt, dict(Cin_p=8192, Cout_p=2048)),               # the GEMM's N is 4 Cout_p
        ('igemm: bad dtype', dict(dtype=NODT)),
        ('igemm: grid out of range', dict(B=big >> 2, Cout_p=64))])
    refused('clamd_convT2x2_fwd', _CT_FWD, ct, padded, Cout_p=12)
    dg = dict(gy=None, gy_ldc=64, w=None, gx=None, gx_ldc=64, bn_y=None, bn_sums=None, stat_rows=0, B=1, H=32, W=32, Cin_p=64, Cout_p=64, dtype=F32,
              stream=None)
    n = 'convT2x2_dgrad: '
    chain('clamd_convT2x2_dgrad', _CT_DGRAD, dg, [
        ('igemm: empty problem', dict(H=0)),
        (split, dict(dtype=SPLIT, gy=odd)),
        (padded, dict(Cin_p=40)),
        (image, dict(H=2048, W=2048, gy_ldc=32, gx_ldc=8)),
        (out_image, dict(H=2048, W=2048, gy_ldc=8, gx_ldc=32)),
        (filt, dict(Cin_p=8192, Cout_p=2048)),
        (n + 'bn_y and bn_sums go together', dict(bn_y=p, bn_sums=None)),
        (rows % ('convT2x2_dgrad', 7, 4), dict(bn_y=p, bn_sums=p, stat_rows=7)),
        ('igemm: bad dtype', dict(dtype=NODT)),
        ('igemm: grid out of range', dict(B=big >> 2, Cin_p=256))])
    refused('clamd_convT2x2_dgrad', _CT_DGRAD, dg, n + 'bn_y and bn_sums go together', bn_sums=p)
    refused('clamd_convT2x2_dgrad', _CT_DGRAD, dg, split, dtype=SPLIT, bn_y=p, bn_sums=p, Cin_p=40)
    # The image bounds count 4 H W pixels for the data gradient alone, for both of its images (its INPUT is the 2H x 2W one); the forward
    # launch, whose OUTPUT is 2H x 2W, is bounded as H x W.  2048 x 2048 x 32 channels: 2^29 bytes as H x W, 2^31 as 2H x 2W.
    refused('clamd_convT2x2_fwd', _CT_FWD, ct, 'igemm: bad dtype', H=2048, W=2048, x_ldc=32, y_ldc=32, dtype=NODT)
    refused('clamd_convT2x2_dgrad', _CT_DGRAD, dg, image, H=2048, W=2048, gy_ldc=32, gx_ldc=32, dtype=NODT)

    wg = dict(mode=0, a=None, a_ldc=64, b=None, b_ldc=64, ws=None, ws_bytes=0, out=None, B=1, H=32, W=32, Rp=64, Cp=64, R=64, C=64, r_seg0=64,
              r_seg0p=64, c_seg0=64, c_seg0p=64, dtype=F32, tune=None, stream=None)
    n = 'wgrad: '
    chain('clamd_wgrad', _WG, wg, [
        (n + 'bad mode', dict(mode=3)),
        tuning,
        (n + 'channel counts/pitches must be padded', dict(Rp=48)),
        (n + 'empty problem', dict(B=0)),
        (split, dict(dtype=SPLIT, a=odd)),
        (n + 'one image exceeds 2^30 bytes', dict(H=2048, W=2048)),
        (n + 'workspace too small', dict(ws_bytes=16 * 9 * 64 * 64 * 4 - 1)),
        (n + 'bad dtype', dict(dtype=NODT, ws_bytes=1 << 40))])
    refused('clamd_wgrad', _WG, wg, n + 'bad mode', mode=-1)
    for kw in (dict(Cp=40), dict(a_ldc=68), dict(b_ldc=68)):
        refused('clamd_wgrad', _WG, wg, n + 'channel counts/pitches must be padded', **kw)
    for kw in (dict(b=odd), dict(a=p, a_ldc=72), dict(b=p, b_ldc=72)):
        refused('clamd_wgrad', _WG, wg, split, dtype=SPLIT, **kw)
    # the ConvTranspose2d gradient's B operand lives on the 2H x 2W grid
    refused('clamd_wgrad', _WG, wg, n + 'one image exceeds 2^30 bytes', mode=2, H=1024, W=1024, a_ldc=8)
    refused('clamd_wgrad', _WG, wg, n + 'one image exceeds 2^30 bytes', H=2048, W=2048, b_ldc=8)
    # slabs of the split-K plan: fp32 32 x 32 -> 16 tiles of 2 x 32 (the 16 splits above), of 4 x 16 with wgrad_tw16; the 2-per-CU
    # kernel (wgrad_ws = 0) takes twice the slabs of the producer/consumer one when the tiles allow; 1x1 and 2x2 forms have 1 and 4 taps
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', H=64, W=64, ws_bytes=64 * 9 * 64 * 64 * 4 - 1, tune=tref(wgrad_ws=0))
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', H=64, W=64, Rp=256, Cp=256, ws_bytes=16 * 9 * 256 * 256 * 4 - 1)
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', H=64, W=64, Rp=256, Cp=256, ws_bytes=32 * 9 * 256 * 256 * 4 - 1, tune=tref(wgrad_ws=0))
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', mode=1, ws_bytes=16 * 64 * 64 * 4 - 1)
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', mode=2, ws_bytes=32 * 4 * 64 * 64 * 4 - 1)
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', dtype=1, ws_bytes=8 * 9 * 64 * 64 * 4 - 1)
    refused('clamd_wgrad', _WG, wg, n + 'workspace too small', ws_bytes=9 * 64 * 64 * 4 - 1, tune=tref(wgrad_blocks=1))

    sr = dict(op=ops['conv1x1'], B=1, H=32, W=32, Cin_p=64, Cout_p=64, dtype=F32, fused_bn=0, tune=None)
    n = 'stat_rows: '
    chain('clamd_stat_rows', _ROWS, sr, [
        (n + 'empty problem', dict(Cout_p=0)),
        tuning,
        (n + 'unknown op', dict(op=99)),
        (n + 'out of range', dict(B=big))])
    for kw in (dict(B=0), dict(H=-1), dict(W=0)):
        refused('clamd_stat_rows', _ROWS, sr, n + 'empty problem', **kw)
    refused('clamd_stat_rows', _ROWS, sr, n + 'out of range', op=ops['convT_dgrad'], B=big)
    for t in (direct, ws1):
        refused('clamd_stat_rows', _ROWS, sr, n + 'out of range', op=ops['conv3x3'], B=big, tune=t)


_CE = 'logits labels old_logits K_old_total c_old temperature lam dlogits loss3 ws ws_bytes B K H W ignore_index grad_scale stream'.split()
_CE_COUNT = 'labels B K H W ignore_index ws ws_bytes stream'.split()
_CE_COUNTED = 'logits labels dlogits dl_nhwc dl_ldc dl_dtype loss3 ws ws_bytes B K H W ignore_index grad_scale stream'.split()
_CE_WEIGHTED = 'logits labels image_weight dlogits dl_nhwc dl_ldc dl_dtype loss3 ws ws_bytes B K H W ignore_index grad_scale stream'.split()
_CE_UNBIASED = ('logits labels old_logits K_old_total c_old lam dlogits dl_nhwc dl_ldc dl_dtype loss3 ws ws_bytes B K H W ignore_index grad_scale '
                'stream').split()
_CE_CLASS = ('logits labels class_weight image_weight dlogits dl_nhwc dl_ldc dl_dtype loss3 ws ws_bytes B K H W ignore_index label_smoothing '
             'focal_gamma grad_scale stream').split()
_CE_DICE = ('logits labels dlogits dl_nhwc dl_ldc dl_dtype loss3 ws ws_bytes B K H W ignore_index w_ce w_dice smooth first_class present_only '
            'per_image grad_scale stream').split()


def test_loss_entry_points_refuse_with_pinned_messages(C):
    """Every refusal of the seven per-pixel loss entry points (loss.hip) that returns before any launch, with the WHOLE message and status
    -1; consecutive checks are also violated together and the earlier one answers.  The two workspace queries and the counter's offset are
    pinned as numbers.  Nothing here passes validation: no pointer is dereferenced and nothing is launched."""
    lib = C._lib.load()
    refused, chain = _refusal_tools(lib)
    p, odd = 0x1000, 0x1010                                 # 64-byte aligned / 16-byte aligned only
    F32, SPLIT, NODT = 0, 2, 9
    ce_ws, class_ws = 18448, 53408
    assert lib.clamd_ce_workspace_bytes() == ce_ws and lib.clamd_ce_class_workspace_bytes() == class_ws
    assert lib.clamd_ce_bad_label_count_offset() == 16388
    # the Dice workspace: the CE workspace, B * min(ceil(HW / 256), 2048 // B) rows of 100 words, 64 words and a double per group
    dice_ws = lib.clamd_ce_dice_workspace_bytes
    assert [dice_ws(2, 5, 8, 12, g) for g in (0, 1)] == [ce_ws + 4 * (2 * 100 + 64 + 2), ce_ws + 4 * (2 * 100 + 2 * 64 + 4)]
    assert dice_ws(9, 21, 484, 484, 1) == ce_ws + 4 * (9 * 227 * 100 + 9 * 64 + 18) and dice_ws(2048, 32, 1, 1, 0) == ce_ws + 4 * (2048 * 100 + 66)
    assert [dice_ws(*a) for a in ((2049, 5, 8, 12, 0), (2, 0, 8, 12, 0), (2, 33, 8, 12, 0), (0, 5, 8, 12, 0), (2, 5, 0, 12, 0), (2, 5, 8, 0, 1))] == [0] * 6

    split = 'bf16x3 tensors need a 64-byte aligned base and a pitch that is a multiple of 16 channels'
    small = 'ce: workspace too small'

    def plan(who, nhwc=True, ws_step=True):
        """ce_plan's checks in their order"""
        steps = [(who + ': null pointer or empty shape', dict(B=0)), (who + ': number of classes must be in [1, 32]', dict(K=33))]
        if ws_step:
            steps.append((small, dict(ws_bytes=ce_ws - 1)))
        steps.append((who + ': misaligned tensor', dict(labels=0x1004)))
        if nhwc:
            steps += [(who + ': the NHWC copy needs a pitch >= 32 channels, a multiple of 8, and a 16-byte aligned base', dict(dl_nhwc=p, dl_ldc=24)),
                      (who + ': bad dtype', dict(dl_nhwc=p, dl_dtype=NODT)),
                      (split, dict(dl_nhwc=odd, dl_dtype=SPLIT))]
        return steps

    def plan_singles(name, order, base, who, nhwc=True, k0=None):
        for k in ('logits', 'labels', 'dlogits', 'loss3', 'ws'):
            refused(name, order, base, who + ': null pointer or empty shape', **{k: None})
        for kw in (dict(H=0), dict(W=-1), dict(B=-3)):
            refused(name, order, base, who + ': null pointer or empty shape', **kw)
        refused(name, order, base, k0 or who + ': number of classes must be in [1, 32]', K=0)
        for kw in (dict(logits=0x1002), dict(dlogits=0x1001)):
            refused(name, order, base, who + ': misaligned tensor', **kw)
        if nhwc:
            for kw in (dict(dl_ldc=36), dict(dl_nhwc=0x1008)):
                refused(name, order, base, who + ': the NHWC copy needs a pitch >= 32 channels, a multiple of 8, and a 16-byte aligned base',
                        **{'dl_nhwc': p, **kw})
            refused(name, order, base, split, dl_nhwc=p, dl_dtype=SPLIT, dl_ldc=40)

    shape = dict(B=2, K=5, H=8, W=12, ignore_index=-100, grad_scale=1.0, stream=None)
    common = dict(shape, logits=p, labels=p, dlogits=p, loss3=p, ws=p, ws_bytes=1 << 26)
    nhwc = dict(common, dl_nhwc=None, dl_ldc=32, dl_dtype=F32)

    ce = dict(common, old_logits=None, K_old_total=0, c_old=0, temperature=2.0, lam=1.0)
    chain('clamd_ce_fwd_bwd', _CE, ce, plan('ce', nhwc=False) + [('ce: bad c_old', dict(old_logits=p, c_old=0))])
    plan_singles('clamd_ce_fwd_bwd', _CE, ce, 'ce', nhwc=False)
    refused('clamd_ce_fwd_bwd', _CE, ce, 'ce: misaligned tensor', old_logits=0x1002, c_old=1, K_old_total=5)
    for kw in (dict(c_old=6, K_old_total=8), dict(c_old=3, K_old_total=2)):
        refused('clamd_ce_fwd_bwd', _CE, ce, 'ce: bad c_old', old_logits=p, **kw)

    cnt = dict(shape, labels=p, ws=p, ws_bytes=1 << 26)
    chain('clamd_ce_count', _CE_COUNT, cnt, [('ce_count: bad arguments', dict(K=0)), (small, dict(ws_bytes=ce_ws - 1))])
    for kw in (dict(K=33), dict(labels=None), dict(B=0), dict(H=0), dict(W=0)):
        refused('clamd_ce_count', _CE_COUNT, cnt, 'ce_count: bad arguments', **kw)

    who = 'ce_fwd_bwd_counted'
    four = who + ': needs H * W % 4 == 0 and 16-byte aligned logits / 32-byte aligned labels (use clamd_ce_fwd_bwd)'
    chain('clamd_ce_fwd_bwd_counted', _CE_COUNTED, nhwc, plan(who) + [(four, dict(H=7, W=9))])
    plan_singles('clamd_ce_fwd_bwd_counted', _CE_COUNTED, nhwc, who)
    for kw in (dict(logits=0x1004), dict(dlogits=0x1008), dict(labels=0x1010)):
        refused('clamd_ce_fwd_bwd_counted', _CE_COUNTED, nhwc, four, **kw)

    who = 'ce_weighted'
    need = who + ': image_weight (B floats) is required (clamd_ce_fwd_bwd_counted is the unweighted loss)'
    wce = dict(nhwc, image_weight=p)
    chain('clamd_ce_fwd_bwd_weighted', _CE_WEIGHTED, wce, [(need, dict(image_weight=None))] + plan(who))
    refused('clamd_ce_fwd_bwd_weighted', _CE_WEIGHTED, wce, need, image_weight=0x1002)
    plan_singles('clamd_ce_fwd_bwd_weighted', _CE_WEIGHTED, wce, who)

    who = 'ce_unbiased'
    exceeds = dict(old_logits=p, K_old_total=1, c_old=2)
    uce = dict(nhwc, old_logits=None, K_old_total=0, c_old=1, lam=1.0)
    chain('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, [
        (who + ': c_old must be in [1, K]', dict(c_old=0)),
        (who + ': lam must be >= 0', dict(lam=-1.0)),
        (who + ": c_old exceeds the old model's class count K_old_total", exceeds)] + plan(who))
    refused('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, who + ': c_old must be in [1, K]', c_old=6)
    refused('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, who + ': lam must be >= 0', lam=float('nan'))
    # lam == 0 drops the old model before its checks: neither its class count nor its alignment is looked at
    refused('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, who + ': null pointer or empty shape', lam=0.0, B=0, **exceeds)
    refused('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, who + ': null pointer or empty shape', lam=0.0, B=0, old_logits=0x1002)
    refused('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, who + ': misaligned tensor', old_logits=0x1002, K_old_total=5)
    plan_singles('clamd_ce_unbiased_fwd_bwd', _CE_UNBIASED, uce, who, k0=who + ': c_old must be in [1, K]')      # c_old = 1 > K answers first

    who = 'ce_class'
    cls_ws = who + ': workspace too small (clamd_ce_class_workspace_bytes) or not 8-byte aligned'
    cce = dict(nhwc, class_weight=p, image_weight=None, label_smoothing=0.0, focal_gamma=0.0)
    chain('clamd_ce_class_fwd_bwd', _CE_CLASS, cce, [
        (who + ': class_weight (K floats) is required and must be 4-byte aligned', dict(class_weight=None)),
        (who + ': misaligned image_weight', dict(image_weight=0x1002)),
        (who + ': label_smoothing must be in [0, 1)', dict(label_smoothing=1.0)),
        (who + ': focal_gamma must be finite and >= 0', dict(focal_gamma=-1.0)),
        (who + ': label_smoothing and focal_gamma are both non-zero: the combination is not defined', dict(label_smoothing=0.1, focal_gamma=0.5)),
        (cls_ws, dict(ws_bytes=class_ws - 1))] + plan(who, ws_step=False))
    refused('clamd_ce_class_fwd_bwd', _CE_CLASS, cce, who + ': class_weight (K floats) is required and must be 4-byte aligned', class_weight=0x1002)
    for v in (-0.1, float('nan')):
        refused('clamd_ce_class_fwd_bwd', _CE_CLASS, cce, who + ': label_smoothing must be in [0, 1)', label_smoothing=v)
    for v in (float('inf'), float('nan')):
        refused('clamd_ce_class_fwd_bwd', _CE_CLASS, cce, who + ': focal_gamma must be finite and >= 0', focal_gamma=v)
    refused('clamd_ce_class_fwd_bwd', _CE_CLASS, cce, cls_ws, ws=0x1004)
    plan_singles('clamd_ce_class_fwd_bwd', _CE_CLASS, cce, who)

    who = 'ce_dice'
    dice_small = who + ': workspace too small (clamd_ce_dice_workspace_bytes)'
    dce = dict(nhwc, w_ce=1.0, w_dice=1.0, smooth=1e-5, first_class=0, present_only=1, per_image=0)
    chain('clamd_ce_dice_fwd_bwd', _CE_DICE, dce, [
        (who + ': first_class must be 0 or 1', dict(first_class=2)),
        (who + ': w_ce, w_dice and smooth must be finite and >= 0', dict(w_ce=-1.0)),
        (dice_small, dict(ws_bytes=ce_ws - 1))] + plan(who, ws_step=False) + [
        (who + ': more than 2048 images: every image needs a partial row of its own and the coefficient pass adds at most 2048', dict(B=2049)),
        (dice_small, dict(ws_bytes=dice_ws(2, 5, 8, 12, 0) - 1)),
        (who + ': workspace must be 16-byte aligned', dict(ws=0x1008))])
    refused('clamd_ce_dice_fwd_bwd', _CE_DICE, dce, who + ': first_class must be 0 or 1', first_class=-1)
    for kw in (dict(w_dice=float('inf')), dict(smooth=float('nan')), dict(w_dice=-0.5), dict(smooth=-1e-9), dict(w_ce=float('inf'))):
        refused('clamd_ce_dice_fwd_bwd', _CE_DICE, dce, who + ': w_ce, w_dice and smooth must be finite and >= 0', **kw)
    refused('clamd_ce_dice_fwd_bwd', _CE_DICE, dce, dice_small, per_image=1, ws_bytes=dice_ws(2, 5, 8, 12, 1) - 1)
    plan_singles('clamd_ce_dice_fwd_bwd', _CE_DICE, dce, who)


def test_abi_rejects_bad_arguments_before_any_launch(C):
    """Error behaviour of the C ABI: argument validation happens on the host before anything is
    enqueued, the entry point returns a negative status, clamd_last_error() names the problem and the Python side raises
    RuntimeError — as the reference's failures surface as Python exceptions (unet.py:88-91).  No GPU needed: every call
    below must fail validation (null pointers are never dereferenced)."""
    lib = C._lib.load()
    call = C._lib.call
    keep = []                            # Tuning objects passed by address stay alive until the test ends

    def tref(**kw):
        keep.append(C._lib.Tuning(**kw))
        return keep[-1].ref()

    cases = [
        ('empty problem', 'clamd_conv3x3', (None, 32, None, None, None, 32, None, None, None, 0, 0, 16, 16, 32, 32, 1, 0, 0, None, None)),
        ('padded', 'clamd_conv3x3', (None, 32, None, None, None, 32, None, None, None, 0, 1, 16, 16, 24, 32, 1, 0, 0, None, None)),
        ('bad dtype', 'clamd_conv3x3', (None, 32, None, None, None, 32, None, None, None, 0, 1, 16, 16, 32, 32, 1, 0, 9, None, None)),
        ('partial rows', 'clamd_conv3x3', (None, 32, None, None, None, 32, 1, None, None, 5, 1, 16, 16, 32, 32, 1, 0, 0, None, None)),
        ('empty problem', 'clamd_conv3x3_winograd', (None, 32, None, None, None, 32, None, 0, 1, 0, 16, 32, 32, 1, None, None)),
        ('must be even', 'clamd_conv3x3_winograd', (None, 32, None, None, None, 32, None, 0, 1, 15, 16, 32, 32, 1, None, None)),
        ('padded', 'clamd_conv3x3_winograd', (None, 32, None, None, None, 32, None, 0, 1, 16, 16, 40, 32, 1, None, None)),
        ('stat_rows', 'clamd_conv3x3_winograd', (None, 32, None, None, None, 32, 1, 7, 1, 16, 16, 32, 32, 1, None, None)),
        ('must be even', 'clamd_wgrad_winograd', (None, 32, None, 32, None, 0, None, 1, 16, 17, 32, 32, 32, 32, 32, 32, 32, 32, None, None)),
        ('workspace too small', 'clamd_wgrad_winograd', (None, 32, None, 32, None, 0, None, 1, 16, 16, 32, 32, 32, 32, 32, 32, 32, 32, None, None)),
        ('bad mode', 'clamd_wgrad', (7, None, 32, None, 32, None, 0, None, 1, 16, 16, 32, 32, 32, 32, 32, 32, 32, 32, 0, None, None)),
        ('empty problem', 'clamd_wgrad', (0, None, 32, None, 32, None, 0, None, 0, 16, 16, 32, 32, 32, 32, 32, 32, 32, 32, 0, None, None)),
        ('stat_rows', 'clamd_bn_finalize', (1, 0, None, None, None, None, None, None, None, None, 32, 32, 1.0, 0.1, 1e-5, None, None)),
        ('sum_rows', 'clamd_bn_bwd_reduce', (1, 32, None, 0, 1, 32, None, None, 1, 3, 1, 16, 16, 32, 0, None, None)),
        ('workspace too small', 'clamd_channel_sum', (1, 32, 1, 64, 32, 32, 0, None, 0, None, None)),
        ('empty job table', 'clamd_wino_pack', (None, 0, 0, None)),
        ('bad relu flags', 'clamd_conv3x3', (None, 32, None, None, None, 32, None, None, None, 0, 1, 16, 16, 32, 32, 4, 0, 0, None, None)),
        ('bn_y and bn_sums go together', 'clamd_conv3x3', (None, 32, None, None, None, 32, None, 0x1000, None, 0, 1, 16, 16, 32, 32, 0, 0, 0, None, None)),
        ('bn_y and bn_sums go together', 'clamd_conv3x3', (None, 32, None, None, None, 32, None, None, 0x1000, 4, 1, 16, 16, 32, 32, 0, 0, 0, None, None)),
        ('padded', 'clamd_conv3x3', (None, 36, None, None, None, 32, None, None, None, 0, 1, 16, 16, 32, 32, 1, 0, 0, None, None)),
        ('padded', 'clamd_conv3x3', (None, 32, None, None, None, 36, None, None, None, 0, 1, 16, 16, 32, 32, 1, 0, 0, None, None)),
        # Kp = 48: the persistent kernel's own "K-steps in pairs" rule (Kp % 32 in fp32) can never be what declines a shape
        ('padded', 'clamd_conv3x3', (None, 48, None, None, None, 32, None, None, None, 0, 1, 16, 16, 48, 32, 1, 0, 0, None, None)),
        ('border-class bias table', 'clamd_conv3x3', (None, 64, None, None, None, 64, None, None, None, 0, 1, 16, 16, 64, 64, 3, 0, 0, None, None)),
        ('padded', 'clamd_wgrad', (0, None, 40, None, 32, None, 0, None, 1, 16, 16, 40, 32, 40, 32, 40, 40, 32, 32, 0, None, None)),
        ('padded', 'clamd_wgrad', (0, None, 32, None, 36, None, 0, None, 1, 16, 16, 32, 32, 32, 32, 32, 32, 32, 32, 0, None, None)),
        ('workspace too small', 'clamd_wgrad', (0, None, 32, None, 32, None, 0, None, 1, 16, 16, 32, 32, 32, 32, 32, 32, 32, 32, 0, None, None)),
        ('workspace too small', 'clamd_wgrad', (2, None, 32, None, 32, None, 4 * 4 * 32 * 32 - 1, None, 1, 2, 16, 32, 32, 32, 32, 32, 32, 32, 32, 1,
                                                tref(wgrad_blocks=1), None)),
    ]
    for needle, name, args in cases:
        with pytest.raises(RuntimeError) as e:
            call(name, *args)
        assert needle in str(e.value), (name, str(e.value))
        assert needle in lib.clamd_last_error().decode()
    keep.append(C._lib.Tuning())
    keep[-1].wino_mt = 7                 # out of range
    bad_tune = keep[-1].ref()
    _check_winograd_refusals(lib, tref, bad_tune)
    _check_direct_conv_refusals(lib, tref, bad_tune, dict(conv3x3=C._lib.OP_CONV3X3, conv1x1=C._lib.OP_CONV1X1, convT_dgrad=C._lib.OP_CONVT2X2_DGRAD))
    # clamd_conv3x3_border_bias_ok / clamd_conv3x3_bn_sums / clamd_stat_rows(CLAMD_OP_CONV3X3) over the branches of plan_conv3x3 and pws_rows:
    # the persistent kernel takes igemm_pws 2, or 1 up to 256 input channels; K-steps in pairs (Kp % 64 in bf16); bn_y only in bf16
    ok = lambda H, W, Kp, dt, **kw: lib.clamd_conv3x3_border_bias_ok(2, H, W, Kp, 64, dt, tref(**kw) if kw else None)
    assert [ok(16, 16, 64, dt) for dt in (0, 1, 2)] == [1, 1, 1]
    assert [ok(16, 16, Kp, 1) for Kp in (32, 64, 96, 128, 256, 512)] == [0, 1, 0, 1, 1, 0]
    assert [ok(16, 16, Kp, 0) for Kp in (32, 96, 256, 288)] == [1, 1, 1, 0] and ok(16, 16, 512, 0, igemm_pws=2) == 1
    assert ok(16, 16, 64, 0, igemm_pws=0) == 0 and ok(16, 16, 64, 0, igemm_pws=0, igemm_ws=1) == 0
    assert ok(1, 16, 64, 0) == 0 and ok(16, 1, 64, 0) == 0 and ok(2, 2, 64, 0) == 1
    assert lib.clamd_conv3x3_border_bias_ok(0, 16, 16, 64, 64, 0, None) == 0
    bad = C._lib.Tuning()
    bad.igemm_pws = 3
    assert lib.clamd_conv3x3_border_bias_ok(2, 16, 16, 64, 64, 0, bad.ref()) == 0 and lib.clamd_conv3x3_bn_sums(2, 16, 16, 64, 64, 1, bad.ref()) == 0
    sums = lambda Kp, dt, **kw: lib.clamd_conv3x3_bn_sums(2, 16, 16, Kp, 64, dt, tref(**kw) if kw else None)
    assert [sums(64, dt) for dt in (0, 1, 2)] == [5, 2, 5]
    assert [sums(Kp, 1) for Kp in (32, 64, 96, 256, 512)] == [5, 2, 5, 2, 5] and sums(512, 1, igemm_pws=2) == 2 and sums(64, 1, igemm_pws=0) == 5
    assert lib.clamd_conv3x3_bn_sums(0, 16, 16, 64, 64, 1, None) == 0 and lib.clamd_conv3x3_bn_sums(2, 16, 0, 64, 64, 1, None) == 0
    rows = lambda shape, Kp, Np, dt, bn, **kw: lib.clamd_stat_rows(C._lib.OP_CONV3X3, *shape, Kp, Np, dt, bn, tref(**kw))
    assert rows((2, 40, 128), 64, 256, 0, 0, igemm_pws=2, cu_reserve=128) == 32           # (256 - 128) CUs / 4 slabs
    assert rows((2, 40, 128), 64, 256, 0, 0, igemm_pws=2, cu_reserve=0) == 40            # clamped to the 40 tiles
    assert rows((2, 40, 128), 64, 256, 0, 1, igemm_pws=2, igemm_ws=0, cu_reserve=128) == 40      # fp32 declines bn_y: the baseline's tiles
    assert rows((2, 40, 128), 64, 256, 1, 1, igemm_pws=2, igemm_ws=0, cu_reserve=128) == 32
    assert rows((2, 40, 128), 32, 256, 1, 0, igemm_pws=2, igemm_ws=3, cu_reserve=128) == 2 * 3 * 4    # bf16 declines Kp 32: 512-pixel tiles
    assert [rows((2, 17, 18), 64, 64, 0, 0, igemm_pws=0, igemm_ws=w) for w in (0, 1, 3, 4)] == [8, 8, 8, 12]      # W < 32: 512-pixel tiles clamp to 256
    assert [rows((1, 9, 36), 64, 64, 0, 0, igemm_pws=0, igemm_ws=w) for w in (0, 1, 3, 4)] == [4, 4, 2, 6]


@pytest.fixture
def conv3_grid(monkeypatch):
    """tests/test_conv3_grid_gpu.py with its tensors on the host: its case lists, its copies of the launchers' rules and its float64
    references need no device, only its launches and comparisons do."""
    import grid_util
    import test_conv3_grid_gpu as grid
    for mod in (grid_util, grid):
        monkeypatch.setattr(mod, 'DEV', torch.device('cpu'))
    return grid


def test_conv3_grid_cases_reach_every_instantiation(conv3_grid):
    """The rows of test_conv3_grid_gpu.py start every kernel instantiation its path table names: all 8 (fp32, bf16x3) and 16 (bf16) of
    launch_pws_t, every baseline and producer/consumer one, every reduce kernel and split class of clamd_wgrad."""
    conv3_grid.check_conv3x3_plans()
    conv3_grid.check_wgrad_plans()


def test_conv3_grid_exact_cases_stay_below_2_24(conv3_grid):
    """Every exact-integer case of test_conv3_grid_gpu.py keeps every sum of absolute terms below 2^24, from its references alone."""
    conv3_grid.check_exact_conditions()


@pytest.fixture
def wino_grid(monkeypatch):
    """tests/test_wino_wgrad_grid_gpu.py with its tensors on the host (as conv3_grid)."""
    import grid_util
    import test_wino_wgrad_grid_gpu as grid
    for mod in (grid_util, grid):
        monkeypatch.setattr(mod, 'DEV', torch.device('cpu'))
    return grid


def test_wino_wgrad_grid_cases_reach_every_plan(wino_grid):
    """The rows of test_wino_wgrad_grid_gpu.py reach both in-kernel kernels ragged and not, every reduce template and split class, every
    stream-K slot class, the wave-level plan's four block shapes and the default plan's switch, from its copies of the launchers' rules."""
    wino_grid.check_wino_wgrad_plans()


def test_wino_wgrad_grid_exact_cases_stay_below_2_24(wino_grid):
    """Every exact-integer case keeps every transform and plane sum of absolute terms below 2^24, and the file's transform matrices
    reproduce the direct-sum reference in float64, from the references alone."""
    wino_grid.check_wino_exact_conditions()


def test_wino_wgrad_grid_layout_helpers_round_trip(wino_grid):
    """The V / Yt index helpers and the tile order of test_wino_wgrad_grid_gpu.py round-trip and agree with the vectorised placement."""
    wino_grid.check_wino_layout_helpers()


@pytest.fixture
def wino_fwd_grid(monkeypatch):
    """tests/test_wino_pre_fwd_grid_gpu.py with its tensors on the host (as conv3_grid)."""
    import grid_util
    import test_wino_pre_fwd_grid_gpu as grid
    for mod in (grid_util, grid):
        monkeypatch.setattr(mod, 'DEV', torch.device('cpu'))
    return grid


def test_wino_pre_fwd_grid_cases_reach_every_plan(wino_fwd_grid):
    """The rows of test_wino_pre_fwd_grid_gpu.py reach all four instantiations of both forward kernels with every K-loop length, every
    output width and pitch, and the persistent grid's item classes (two and three items, a slab change, one item, both forced bands)."""
    wino_fwd_grid.check_wino_fwd_plans()


def test_wino_pre_fwd_grid_exact_cases_stay_below_2_24(wino_fwd_grid):
    """Every hand-placed case keeps every output element and every row's first moments (the low-magnitude cases: the second moments too)
    below 2^24, and the file's matrices and layouts reproduce the nine-tap direct sums in float64, from the references alone."""
    wino_fwd_grid.check_wino_fwd_exact_conditions()


def test_wino_pre_fwd_grid_layout_helpers_round_trip(wino_fwd_grid):
    """The packed-filter index helpers round-trip and agree with the vectorised placement; tiles land where the tile order says."""
    wino_fwd_grid.check_wino_fwd_layout_helpers()


def test_bn_launchers_reject_null_pointers_short_pitches_and_empty_sizes(C):
    """clamd_bn_finalize / _apply / _bwd_reduce / _bwd_finalize / _bwd_apply / _bwd_apply_sums / _bwd_eval, clamd_maxpool2x2[_bwd] and
    clamd_channel_sum: a null pointer the selected kernel would dereference, a pitch below Cp, a non-positive B / H / W are refused by a host check -- status -1 (clamd_fail) and that check's message, never -2 (a launch
    that was tried).  The optional pointers stay optional: those calls are not made here, the GPU suite makes them."""
    import ctypes
    lib = C._lib.load()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every case below fails its checks on the host

    def refused(name, needle, order, base, **kw):
        a = dict(base)
        a.update(kw)
        rc = getattr(lib, name)(*[a[k] for k in order])
        msg = lib.clamd_last_error().decode()
        assert rc == -1 and msg.startswith(name[len('clamd_'):] + ': ') and needle in msg, (name, kw, rc, msg)

    fin = 'stats stat_rows gamma beta running_mean running_var scale shift save_mean save_istd Cp C count momentum eps nbt stream'.split()
    base = dict(stats=p, stat_rows=4, gamma=p, beta=p, running_mean=p, running_var=p, scale=p, shift=p, save_mean=p, save_istd=p, Cp=64, C=60,
                count=8.0, momentum=0.1, eps=1e-5, nbt=None, stream=None)
    for k in ('gamma', 'beta', 'scale', 'shift', 'save_mean', 'save_istd'):
        refused('clamd_bn_finalize', 'null argument', fin, base, **{k: None})
    refused('clamd_bn_finalize', 'running_mean and running_var go together', fin, base, running_var=None)
    refused('clamd_bn_finalize', 'running_mean and running_var go together', fin, base, running_mean=None)
    refused('clamd_bn_finalize', 'needs the running statistics', fin, base, stats=None, stat_rows=0, running_mean=None, running_var=None)
    refused('clamd_bn_finalize', 'bad channel counts', fin, base, Cp=60)
    refused('clamd_bn_finalize', 'bad channel counts', fin, base, C=65)

    app = 'y y_ldc scale shift out out_ldc pooled p_ldc B H W Cp dtype stream'.split()
    base = dict(y=p, y_ldc=64, scale=p, shift=p, out=p, out_ldc=128, pooled=None, p_ldc=0, B=2, H=8, W=6, Cp=64, dtype=0, stream=None)
    for k in ('y', 'scale', 'shift', 'out'):
        refused('clamd_bn_apply', 'null argument', app, base, **{k: None})
        refused('clamd_bn_apply', 'null argument', app, base, pooled=p, p_ldc=64, **{k: None})
    for kw in (dict(y_ldc=56), dict(out_ldc=32), dict(out_ldc=0), dict(pooled=p, p_ldc=32), dict(y_ldc=-64)):
        refused('clamd_bn_apply', 'pitches must be >= Cp', app, base, **kw)
    for kw in (dict(B=0), dict(H=0), dict(W=-2), dict(B=-1, pooled=p, p_ldc=64)):
        refused('clamd_bn_apply', 'bad sizes', app, base, **kw)
    refused('clamd_bn_apply', 'pooling needs even H, W', app, base, pooled=p, p_ldc=64, W=7)
    refused('clamd_bn_apply', 'power of two', app, base, Cp=48)
    refused('clamd_bn_apply', 'bad dtype', app, base, dtype=5)

    red = 'ga ga_ldc gp gp_ldc y y_ldc scale shift sums sum_rows B H W Cp dtype tune stream'.split()
    rows = lib.clamd_stat_rows(C._lib.OP_BN_BWD_REDUCE, 2, 8, 6, 0, 64, 0, 0, None)
    rows_p = lib.clamd_stat_rows(C._lib.OP_BN_BWD_REDUCE, 2, 8, 6, 1, 64, 0, 0, None)
    assert rows > 0 and rows_p > 0
    base = dict(ga=p, ga_ldc=64, gp=None, gp_ldc=0, y=p, y_ldc=64, scale=None, shift=None, sums=p, sum_rows=rows, B=2, H=8, W=6, Cp=64, dtype=0,
                tune=None, stream=None)
    pooled = dict(gp=p, gp_ldc=64, scale=p, shift=p, sum_rows=rows_p)
    refused('clamd_bn_bwd_reduce', 'no gradient source', red, base, ga=None)
    for k in ('y', 'sums'):
        refused('clamd_bn_bwd_reduce', 'null argument', red, base, **{k: None})
        refused('clamd_bn_bwd_reduce', 'null argument', red, base, **{**pooled, k: None})
    for k in ('scale', 'shift'):                                       # read by the pooled kernel only
        refused('clamd_bn_bwd_reduce', 'null argument', red, base, **{**pooled, k: None})
    for kw in (dict(ga_ldc=32), dict(y_ldc=63), {**pooled, 'gp_ldc': 32}, {**pooled, 'ga_ldc': 8}):
        refused('clamd_bn_bwd_reduce', 'pitches must be >= Cp', red, base, **kw)
    for kw in (dict(B=0), dict(H=-8), dict(W=0)):
        refused('clamd_bn_bwd_reduce', 'bad sizes', red, base, **kw)
    refused('clamd_bn_bwd_reduce', 'pooling needs even H, W', red, base, **{**pooled, 'H': 7})
    refused('clamd_bn_bwd_reduce', 'sum_rows does not match', red, base, sum_rows=rows + 1)
    refused('clamd_bn_bwd_reduce', 'bad dtype', red, base, dtype=3)

    bfin = 'sums sum_rows gamma save_mean save_istd k012 dgamma dbeta dbias Cp C count stream'.split()
    base = dict(sums=p, sum_rows=4, gamma=p, save_mean=p, save_istd=p, k012=p, dgamma=p, dbeta=p, dbias=None, Cp=64, C=60, count=8.0, stream=None)
    for k in ('sums', 'gamma', 'save_mean', 'save_istd', 'k012', 'dgamma', 'dbeta'):
        refused('clamd_bn_bwd_finalize', 'null argument', bfin, base, **{k: None})
        refused('clamd_bn_bwd_finalize', 'null argument', bfin, base, dbias=p, **{k: None})
    refused('clamd_bn_bwd_finalize', 'sum_rows must be', bfin, base, sum_rows=0)
    refused('clamd_bn_bwd_finalize', 'bad channel counts', bfin, base, Cp=60)
    refused('clamd_bn_bwd_finalize', 'bad channel counts', bfin, base, C=65)

    bapp = 'ga ga_ldc gp gp_ldc y y_ldc scale shift k012 gz gz_ldc B H W Cp dtype stream'.split()
    base = dict(ga=p, ga_ldc=64, gp=None, gp_ldc=0, y=p, y_ldc=64, scale=None, shift=None, k012=p, gz=p, gz_ldc=64, B=2, H=8, W=6, Cp=64, dtype=0,
                stream=None)
    pooled = dict(gp=p, gp_ldc=64, scale=p, shift=p)
    refused('clamd_bn_bwd_apply', 'no gradient source', bapp, base, ga=None)
    for k in ('y', 'k012', 'gz'):
        refused('clamd_bn_bwd_apply', 'null argument', bapp, base, **{k: None})
        refused('clamd_bn_bwd_apply', 'null argument', bapp, base, **{**pooled, k: None})
    for k in ('scale', 'shift'):
        refused('clamd_bn_bwd_apply', 'null argument', bapp, base, **{**pooled, k: None})
    for kw in (dict(ga_ldc=32), dict(y_ldc=0), dict(gz_ldc=56), {**pooled, 'gp_ldc': 32}):
        refused('clamd_bn_bwd_apply', 'pitches must be >= Cp', bapp, base, **kw)
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        refused('clamd_bn_bwd_apply', 'bad sizes', bapp, base, **kw)
    refused('clamd_bn_bwd_apply', 'pooling needs even H, W', bapp, base, **{**pooled, 'W': 5})
    refused('clamd_bn_bwd_apply', 'bad dtype', bapp, base, dtype=-1)

    # the other streaming launchers go through the same check: every required pointer, every pitch, each size, the channel rule, the dtype
    # and the row count / workspace the caller sized
    asum = 'ga ga_ldc y y_ldc k012 gz gz_ldc gz_rows nrows B H W Cp dtype stream'.split()
    nr = lib.clamd_bn_bwd_apply_sums_rows(2, 8, 6, 64)
    assert nr > 0
    base = dict(ga=p, ga_ldc=64, y=p, y_ldc=64, k012=p, gz=p, gz_ldc=128, gz_rows=p, nrows=nr, B=2, H=8, W=6, Cp=64, dtype=0, stream=None)
    for k in ('ga', 'y', 'k012', 'gz', 'gz_rows'):
        refused('clamd_bn_bwd_apply_sums', 'null argument', asum, base, **{k: None})
    for kw in (dict(ga_ldc=63), dict(y_ldc=63), dict(gz_ldc=63), dict(gz_ldc=0), dict(y_ldc=-64)):
        refused('clamd_bn_bwd_apply_sums', 'pitches must be >= Cp', asum, base, **kw)
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(H=-8)):
        refused('clamd_bn_bwd_apply_sums', 'bad sizes', asum, base, **kw)
    for cp in (48, 16, 4096):
        refused('clamd_bn_bwd_apply_sums', 'power of two', asum, base, Cp=cp)
    refused('clamd_bn_bwd_apply_sums', 'bad dtype', asum, base, dtype=3)
    for d in (-1, 1):
        refused('clamd_bn_bwd_apply_sums', 'nrows must be', asum, base, nrows=nr + d)

    ev = 'ga ga_ldc gp gp_ldc y y_ldc scale shift gz gz_ldc rows nrows B H W Cp C dtype stream'.split()
    nr, nrp = lib.clamd_bn_bwd_eval_rows(2, 8, 6, 64, 0), lib.clamd_bn_bwd_eval_rows(2, 8, 6, 64, 1)
    assert nr > 0 and nrp > 0
    base = dict(ga=p, ga_ldc=64, gp=None, gp_ldc=0, y=p, y_ldc=64, scale=p, shift=None, gz=p, gz_ldc=64, rows=p, nrows=nr, B=2, H=8, W=6, Cp=64, C=60,
                dtype=0, stream=None)
    pooled = dict(gp=p, gp_ldc=64, shift=p, nrows=nrp)
    refused('clamd_bn_bwd_eval', 'no gradient source', ev, base, ga=None)
    for k in ('y', 'scale', 'gz', 'rows'):
        refused('clamd_bn_bwd_eval', 'null argument', ev, base, **{k: None})
        refused('clamd_bn_bwd_eval', 'null argument', ev, base, **{**pooled, k: None})
    refused('clamd_bn_bwd_eval', 'null argument', ev, base, **{**pooled, 'shift': None})          # read by the pooled kernel only
    for kw in (dict(ga_ldc=63), dict(y_ldc=63), dict(gz_ldc=63), {**pooled, 'gp_ldc': 63}, {**pooled, 'ga': None, 'gp_ldc': 32}):
        refused('clamd_bn_bwd_eval', 'pitches must be >= Cp', ev, base, **kw)
    for kw in (dict(B=0), dict(H=0), dict(W=0), {**pooled, 'B': -1}):
        refused('clamd_bn_bwd_eval', 'bad sizes', ev, base, **kw)
    for kw in (dict(H=7), dict(W=5)):
        refused('clamd_bn_bwd_eval', 'pooling needs even H, W', ev, base, **{**pooled, **kw})
    for kw in (dict(Cp=48), dict(Cp=4096, C=60), dict(C=0), dict(C=65)):
        refused('clamd_bn_bwd_eval', '0 < C <= Cp', ev, base, **kw)
    refused('clamd_bn_bwd_eval', 'bad dtype', ev, base, dtype=3)
    refused('clamd_bn_bwd_eval', 'nrows must be', ev, base, nrows=nr + 1)
    refused('clamd_bn_bwd_eval', 'nrows must be', ev, base, **{**pooled, 'nrows': nrp - 1})

    # the stand-alone pool takes any multiple of 8 channels (Cp = 24 passes the channel rule and is refused for its pitch below)
    mp = 'x x_ldc sign pooled p_ldc B H W Cp dtype stream'.split()
    base = dict(x=p, x_ldc=64, sign=None, pooled=p, p_ldc=64, B=2, H=8, W=6, Cp=64, dtype=0, stream=None)
    mpb = 'x x_ldc sign gp gp_ldc gx gx_ldc B H W Cp dtype stream'.split()
    base_b = dict(x=p, x_ldc=64, sign=None, gp=p, gp_ldc=64, gx=p, gx_ldc=64, B=2, H=8, W=6, Cp=64, dtype=0, stream=None)
    for name, order, b, ptrs, pitches in (('clamd_maxpool2x2', mp, base, ('x', 'pooled'), ('x_ldc', 'p_ldc')),
                                          ('clamd_maxpool2x2_bwd', mpb, base_b, ('x', 'gp', 'gx'), ('x_ldc', 'gp_ldc', 'gx_ldc'))):
        for k in ptrs:
            refused(name, 'null argument', order, b, **{k: None})
        for k in pitches:
            refused(name, 'pitches must be >= Cp', order, b, **{k: 63})
            refused(name, 'pitches must be >= Cp', order, b, Cp=24, **{k: 16})
        for kw in (dict(B=0), dict(H=0), dict(W=0), dict(W=-2)):
            refused(name, 'bad sizes', order, b, **kw)
        for kw in (dict(H=7), dict(W=5)):
            refused(name, 'pooling needs even H, W', order, b, **kw)
        for cp in (60, 4, 0, -8):
            refused(name, 'multiple of 8', order, b, Cp=cp)
        refused(name, 'bad dtype', order, b, dtype=3)

    cs = 'g ldc out npix Cp C dtype workspace ws_bytes tune stream'.split()
    base = dict(g=p, ldc=64, out=p, npix=96, Cp=64, C=60, dtype=0, workspace=p, ws_bytes=3 * 64 * 4, tune=None, stream=None)      # 3 rows of 32 pixels
    for k in ('g', 'out'):
        refused('clamd_channel_sum', 'null argument', cs, base, **{k: None})
    for ldc in (63, 0, -64):
        refused('clamd_channel_sum', 'pitches must be >= Cp', cs, base, ldc=ldc)
    for kw in (dict(npix=0), dict(npix=-1), dict(C=65)):
        refused('clamd_channel_sum', 'bad sizes', cs, base, **kw)
    for cp in (48, 16, 4096):
        refused('clamd_channel_sum', 'power of two', cs, base, Cp=cp, C=8)
    refused('clamd_channel_sum', 'power of two', cs, base, Cp=48)                                   # C = 60 > 48 too: the channel rule answers first
    refused('clamd_channel_sum', 'bad dtype', cs, base, dtype=3)
    refused('clamd_channel_sum', 'workspace too small', cs, base, ws_bytes=3 * 64 * 4 - 1)
    refused('clamd_channel_sum', 'workspace too small', cs, base, workspace=None)


def test_bn_row_counts_follow_one_rule(C):
    """The partial-row counts of the three reducing passes, restated: clamp(ceil(items / per), 1, cap) with cap = the forced grid or
    clamp(budget // Cp, lo, hi).  bn_bwd_reduce and bn_bwd_eval: items = pixels (2x2 windows when pooled), per = the 256 / (Cp / 8) pixel
    rows of a workgroup, (lo, hi, budget) = (256, 1024, 131072) and (256, 2048, 262144); bn_bwd_apply_sums: 16-byte items, 256 per
    workgroup, a flat cap of 2048.  The callers size their buffers with these counts and the launchers refuse any other."""
    L = C._lib
    lib = L.load()

    def rule(items, per, cap):
        return min(max(-(-items // per), 1), cap)

    def cap_of(forced, cp, lo, hi, budget):
        return forced or min(max(budget // cp, lo), hi)

    for cp in (32, 64, 256, 1024, 2048):
        per = max(256 // (cp // 8), 1)
        for B, H, W in ((1, 2, 2), (2, 6, 10), (16, 16, 16), (16, 256, 256), (32, 512, 512)):
            for pooled in (0, 1):
                npix = B * (H // 2) * (W // 2) if pooled else B * H * W
                for forced in (0, 3):
                    got = L.stat_rows(L.OP_BN_BWD_REDUCE, B, H, W, pooled, cp, L.F32, tuning=L.Tuning(bn_reduce_blocks=forced))
                    assert got == rule(npix, per, cap_of(forced, cp, 256, 1024, 131072)), ('reduce', cp, B, H, W, pooled, forced, got)
                got = lib.clamd_bn_bwd_eval_rows(B, H, W, cp, pooled)
                assert got == rule(npix, per, cap_of(0, cp, 256, 2048, 262144)), ('eval', cp, B, H, W, pooled, got)
            got = lib.clamd_bn_bwd_apply_sums_rows(B, H, W, cp)
            assert got == rule(B * H * W * (cp // 8), 256, 2048), ('apply_sums', cp, B, H, W, got)


def test_bf16x3_plane_layout_helpers_roundtrip():
    """ops.split_encode / split_decode (host-side mirror of csrc/common.hip.h Vec8<split_t>): per 16-channel group 16 bf16 hi then 16
    bf16 lo in the bytes of the fp32 tensor; hi = rne_bf16(x), hi + lo reproduces x to ~2^-17 and is a fixed point of decode(encode(.)); a
    16-channel-aligned slice decodes on its own."""
    import torch
    import continual_learning_amd as C
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 5, 48, generator=g) * 3.0
    e = C.ops.split_encode(x)
    assert e.shape == x.shape and e.dtype == torch.float32
    raw = e.view(torch.int16).reshape(2, 3, 5, 3, 2, 16)
    hi = (raw[..., 0, :].to(torch.int32) << 16).view(torch.float32).reshape(x.shape)
    assert torch.equal(hi, x.to(torch.bfloat16).float())
    d = C.ops.split_decode(e)
    assert float((d - x).abs().max() / x.abs().max()) < 2.0 ** -16
    assert torch.equal(C.ops.split_decode(C.ops.split_encode(d)), d)      # hi + lo values are fixed points (the PAIR may differ at a rounding tie)
    assert torch.equal(C.ops.split_decode(e[..., 16:32]), d[..., 16:32])
    z = C.ops.split_encode(torch.zeros(1, 1, 1, 32))
    assert int(z.view(torch.int32).abs().max()) == 0            # zero padding channels are all-zero bytes


def test_no_test_function_is_shadowed():
    """Two `def test_x` in one module: Python keeps the second and the first silently never runs (round 3: test_misuse_errors in
    tests/test_unet_gpu.py).  Every test name must be defined once per file."""
    import collections
    import glob
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    for f in sorted(glob.glob(os.path.join(here, 'test_*.py'))):
        names = re.findall(r'^def (test_\w+)\(', open(f).read(), flags=re.M)
        dup = [n for n, c in collections.Counter(names).items() if c > 1]
        assert not dup, f'{os.path.basename(f)}: defined more than once: {dup}'


def test_bench_step_traffic_reads_the_committed_profile():
    """bench.py's driver line carries the L2-fabric bytes per step (committed PMC profile of the same workload: everything that misses L2,
    Infinity-Cache hits included) beside SURVEY 8d's algorithmic bytes, and HBM bytes as BOUNDS: no counter behind the Infinity Cache exists."""
    sys.path.insert(0, ROOT)
    import bench
    for dtype, e in (('fp32', 4), ('bf16', 2), ('bf16x3', 4)):
        t = bench.step_traffic(dtype, 256, 16, 64, conv_alg_bytes_per_step=6e9)
        assert t is not None and os.path.exists(os.path.join(ROOT, t['traffic_source']))
        assert t['algorithmic_bytes_per_step'] == int(16 * 250e6 * e + 31_044_821 * 28 + 3 * 31_044_821 * e)
        assert abs(t['fabric_over_algorithmic'] - t['l2_fabric_bytes_per_step'] / t['algorithmic_bytes_per_step']) < 1e-3
        assert 1.0 < t['fabric_over_algorithmic'] < 6.0
        lo, hi = t['hbm_bytes_per_step_bounds']
        assert 0 < lo <= hi == t['l2_fabric_bytes_per_step'] and t['mfma_kernels_fabric_bytes_per_step'] > 0
        assert 'hbm_bytes_per_step' not in t            # the counters do not measure that
    t512 = bench.step_traffic('bf16', 512, 32, 64)      # BASELINE configs[4] on one GPU (profiles/*traffic_bf16_512.json)
    assert t512 is not None and 1.0 < t512['fabric_over_algorithmic'] < 6.0
    assert bench.step_traffic('fp32', 128, 16, 64) is None          # no profile of that workload: nothing invented
