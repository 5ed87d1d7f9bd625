"""The kernel plan (continual-learning_amd/plan.py) of UNet(21, 3, 64) at the shapes people run, without building an engine: which kernel
runs each 3x3 unit forward, for its data gradient and for its weight gradient, and where each BatchNorm is reduced and applied.  The
tables below were read from the engine flags of the commit before the planner existed (the same kernels at every shape and switch).
Kernel names: plan.ALGOS ('im2col': the first layer as a pointwise GEMM in both directions; '-': the first unit has no data gradient).
BatchNorm placement: sums_by = the launch that accumulates a unit's backward sums (absent: a reduce pass), fold_src = the unit whose
BatchNorm this unit's input transform applies, fold_a = the unit whose BatchNorm is folded into this unit's filters, pool_fold = the two
readers whose filters take an encoder block's BatchNorm, head_fold = the unit whose BatchNorm the 1x1 head takes.  No kernel runs here."""
import pytest

# config 2, fp32 (the plan of the issue table)
CONFIG2_FP32 = '''
enc1.0        256x256   32   64  im2col     -          im2col
enc1.3        256x256   64   64  f24_direct f24_direct f24
enc2.block.1  128x128   64  128  f24_direct f24        f24
enc2.block.4  128x128  128  128  f44_pre    f44_pre    f44_pre
enc3.block.1   64x64   128  256  f44_pre    f44_pre    f44_pre
enc3.block.4   64x64   256  256  f44_pre    f44_pre    f44_pre
enc4.block.1   32x32   256  512  f44_pre    f24_pre    f44_pre
enc4.block.4   32x32   512  512  f44_pre    f44_pre    f44_pre
dec1.block.0   16x16   512 1024  f24_pre    f22        f24_pre
dec1.block.3   16x16  1024 1024  f24_pre    f24_pre    f24_pre
dec2.block.0   32x32  1024  512  f44_pre    f44_pre    f44_pre
dec2.block.3   32x32   512  512  f44_pre    f44_pre    f44_pre
dec3.block.0   64x64   512  256  f44_pre    f44_pre    f44_pre
dec3.block.3   64x64   256  256  f44_pre    f44_pre    f44_pre
dec4.block.0  128x128  256  128  f44_pre    f44_pre    f44_pre
dec4.block.3  128x128  128  128  f44_pre    f44_pre    f44_pre
last.0        256x256  128   64  f24        f44_pre    f24
last.3        256x256   64   64  f24_direct f24_direct f24
'''
CONFIG2_FP32_BN = {'sums_by': {},
 'fold_src': {'enc2.block.4': 'enc2.block.1',
              'enc3.block.4': 'enc3.block.1',
              'enc4.block.4': 'enc4.block.1',
              'dec1.block.3': 'dec1.block.0',
              'dec2.block.3': 'dec2.block.0',
              'dec3.block.3': 'dec3.block.0',
              'dec4.block.3': 'dec4.block.0'},
 'fold_a': {'enc1.3': 'enc1.0', 'last.3': 'last.0'},
 'pool_fold': {'enc1.3': ('enc2.block.1', 'last.0')},
 'head_fold': ['last.3']}

# config 2, bf16
CONFIG2_BF16 = '''
enc1.0        256x256   32   64  im2col     -          im2col
enc1.3        256x256   64   64  igemm      igemm      igemm
enc2.block.1  128x128   64  128  igemm      igemm      igemm
enc2.block.4  128x128  128  128  igemm      igemm      igemm
enc3.block.1   64x64   128  256  igemm      igemm      igemm
enc3.block.4   64x64   256  256  igemm      igemm      igemm
enc4.block.1   32x32   256  512  igemm      igemm      igemm
enc4.block.4   32x32   512  512  igemm      igemm      igemm
dec1.block.0   16x16   512 1024  igemm      igemm      igemm
dec1.block.3   16x16  1024 1024  igemm      igemm      igemm
dec2.block.0   32x32  1024  512  igemm      igemm      igemm
dec2.block.3   32x32   512  512  igemm      igemm      igemm
dec3.block.0   64x64   512  256  igemm      igemm      igemm
dec3.block.3   64x64   256  256  igemm      igemm      igemm
dec4.block.0  128x128  256  128  igemm      igemm      igemm
dec4.block.3  128x128  128  128  igemm      igemm      igemm
last.0        256x256  128   64  igemm      igemm      igemm
last.3        256x256   64   64  igemm      igemm      igemm
'''
CONFIG2_BF16_BN = {'sums_by': {'enc1.0': 'enc1.3',
             'enc2.block.1': 'enc2.block.4',
             'enc3.block.1': 'enc3.block.4',
             'dec3.block.0': 'dec3.block.3',
             'dec4.block.0': 'dec4.block.3',
             'last.0': 'last.3'},
 'fold_src': {},
 'fold_a': {'enc1.3': 'enc1.0', 'enc2.block.4': 'enc2.block.1', 'dec4.block.3': 'dec4.block.0', 'last.3': 'last.0'},
 'pool_fold': {},
 'head_fold': ['last.3']}

# config 2, bf16x3
CONFIG2_BF16X3 = '''
enc1.0        256x256   32   64  im2col     -          im2col
enc1.3        256x256   64   64  igemm      igemm      igemm
enc2.block.1  128x128   64  128  igemm      igemm      igemm
enc2.block.4  128x128  128  128  igemm      igemm      igemm
enc3.block.1   64x64   128  256  igemm      igemm      igemm
enc3.block.4   64x64   256  256  igemm      igemm      igemm
enc4.block.1   32x32   256  512  igemm      igemm      igemm
enc4.block.4   32x32   512  512  igemm      igemm      igemm
dec1.block.0   16x16   512 1024  igemm      igemm      igemm
dec1.block.3   16x16  1024 1024  igemm      igemm      igemm
dec2.block.0   32x32  1024  512  igemm      igemm      igemm
dec2.block.3   32x32   512  512  igemm      igemm      igemm
dec3.block.0   64x64   512  256  igemm      igemm      igemm
dec3.block.3   64x64   256  256  igemm      igemm      igemm
dec4.block.0  128x128  256  128  igemm      igemm      igemm
dec4.block.3  128x128  128  128  igemm      igemm      igemm
last.0        256x256  128   64  igemm      igemm      igemm
last.3        256x256   64   64  igemm      igemm      igemm
'''
CONFIG2_BF16X3_BN = {'sums_by': {},
 'fold_src': {},
 'fold_a': {'enc1.3': 'enc1.0', 'enc2.block.4': 'enc2.block.1', 'dec4.block.3': 'dec4.block.0', 'last.3': 'last.0'},
 'pool_fold': {},
 'head_fold': ['last.3']}

# config 5 shape, bf16
CONFIG5_BF16 = '''
enc1.0        512x512   32   64  im2col     -          im2col
enc1.3        512x512   64   64  igemm      igemm      igemm
enc2.block.1  256x256   64  128  igemm      igemm      igemm
enc2.block.4  256x256  128  128  igemm      igemm      igemm
enc3.block.1  128x128  128  256  igemm      igemm      igemm
enc3.block.4  128x128  256  256  igemm      igemm      igemm
enc4.block.1   64x64   256  512  igemm      igemm      igemm
enc4.block.4   64x64   512  512  igemm      igemm      igemm
dec1.block.0   32x32   512 1024  igemm      igemm      igemm
dec1.block.3   32x32  1024 1024  igemm      igemm      igemm
dec2.block.0   64x64  1024  512  igemm      igemm      igemm
dec2.block.3   64x64   512  512  igemm      igemm      igemm
dec3.block.0  128x128  512  256  igemm      igemm      igemm
dec3.block.3  128x128  256  256  igemm      igemm      igemm
dec4.block.0  256x256  256  128  igemm      igemm      igemm
dec4.block.3  256x256  128  128  igemm      igemm      igemm
last.0        512x512  128   64  igemm      igemm      igemm
last.3        512x512   64   64  igemm      igemm      igemm
'''
CONFIG5_BF16_BN = {'sums_by': {'enc1.0': 'enc1.3',
             'enc2.block.1': 'enc2.block.4',
             'enc3.block.1': 'enc3.block.4',
             'dec3.block.0': 'dec3.block.3',
             'dec4.block.0': 'dec4.block.3',
             'last.0': 'last.3'},
 'fold_src': {},
 'fold_a': {'enc1.3': 'enc1.0', 'enc2.block.4': 'enc2.block.1', 'dec4.block.3': 'dec4.block.0', 'last.3': 'last.0'},
 'pool_fold': {},
 'head_fold': ['last.3']}

# the reference default (B=2, 512x256), fp32
REFERENCE_FP32 = '''
enc1.0        512x256   32   64  im2col     -          im2col
enc1.3        512x256   64   64  f24_direct f24_direct f24
enc2.block.1  256x128   64  128  f24_direct f24        f24
enc2.block.4  256x128  128  128  f44_pre    f44_pre    f44_pre
enc3.block.1  128x64   128  256  f24_pre    f22        f24
enc3.block.4  128x64   256  256  f24_pre    f24_pre    f24_pre
enc4.block.1   64x32   256  512  f24_pre    f22        f24_pre
enc4.block.4   64x32   512  512  f24_pre    f22        f24_pre
dec1.block.0   32x16   512 1024  f24_pre    f22        f24_pre
dec1.block.3   32x16  1024 1024  f24_pre    f22        f24_pre
dec2.block.0   64x32  1024  512  f24_pre    f24_pre    f24_pre
dec2.block.3   64x32   512  512  f24_pre    f22        f24_pre
dec3.block.0  128x64   512  256  f24_pre    f44_pre    f24_pre
dec3.block.3  128x64   256  256  f24_pre    f24_pre    f24_pre
dec4.block.0  256x128  256  128  f44_pre    f44_pre    f44_pre
dec4.block.3  256x128  128  128  f44_pre    f44_pre    f44_pre
last.0        512x256  128   64  f24        f44_pre    f24
last.3        512x256   64   64  f24_direct f24_direct f24
'''
REFERENCE_FP32_BN = {'sums_by': {},
 'fold_src': {'enc2.block.4': 'enc2.block.1',
              'enc3.block.4': 'enc3.block.1',
              'enc4.block.4': 'enc4.block.1',
              'dec1.block.3': 'dec1.block.0',
              'dec2.block.3': 'dec2.block.0',
              'dec3.block.3': 'dec3.block.0',
              'dec4.block.3': 'dec4.block.0'},
 'fold_a': {'enc1.3': 'enc1.0', 'last.3': 'last.0'},
 'pool_fold': {'enc1.3': ('enc2.block.1', 'last.0')},
 'head_fold': ['last.3']}

# config 2, fp32, WINOGRAD44=False
CONFIG2_FP32_NO_F44 = '''
enc1.0        256x256   32   64  im2col     -          im2col
enc1.3        256x256   64   64  f24_direct f24_direct f24
enc2.block.1  128x128   64  128  f24_direct f24        f24
enc2.block.4  128x128  128  128  f24        f24        f24
enc3.block.1   64x64   128  256  f24_pre    f24        f24
enc3.block.4   64x64   256  256  f24_pre    f24_pre    f24_pre
enc4.block.1   32x32   256  512  f24_pre    f24_pre    f24_pre
enc4.block.4   32x32   512  512  f24_pre    f24_pre    f24_pre
dec1.block.0   16x16   512 1024  f24_pre    f22        f24_pre
dec1.block.3   16x16  1024 1024  f24_pre    f24_pre    f24_pre
dec2.block.0   32x32  1024  512  f24_pre    f24_pre    f24_pre
dec2.block.3   32x32   512  512  f24_pre    f24_pre    f24_pre
dec3.block.0   64x64   512  256  f24_pre    f24_pre    f24_pre
dec3.block.3   64x64   256  256  f24_pre    f24_pre    f24_pre
dec4.block.0  128x128  256  128  f24        f24        f24
dec4.block.3  128x128  128  128  f24        f24        f24
last.0        256x256  128   64  f24        f24_direct f24
last.3        256x256   64   64  f24_direct f24_direct f24
'''
CONFIG2_FP32_NO_F44_BN = {'sums_by': {},
 'fold_src': {'enc3.block.4': 'enc3.block.1',
              'enc4.block.4': 'enc4.block.1',
              'dec1.block.3': 'dec1.block.0',
              'dec2.block.3': 'dec2.block.0',
              'dec3.block.3': 'dec3.block.0'},
 'fold_a': {'enc1.3': 'enc1.0', 'enc2.block.4': 'enc2.block.1', 'dec4.block.3': 'dec4.block.0', 'last.3': 'last.0'},
 'pool_fold': {'enc1.3': ('enc2.block.1', 'last.0')},
 'head_fold': ['last.3']}

# config 2, fp32, FOLD_BN_INTO_FILTERS=False
CONFIG2_FP32_NO_FILTER_FOLD = '''
enc1.0        256x256   32   64  im2col     -          im2col
enc1.3        256x256   64   64  f24_direct f24_direct f24
enc2.block.1  128x128   64  128  f24_direct f24        f24
enc2.block.4  128x128  128  128  f44_pre    f44_pre    f44_pre
enc3.block.1   64x64   128  256  f44_pre    f44_pre    f44_pre
enc3.block.4   64x64   256  256  f44_pre    f44_pre    f44_pre
enc4.block.1   32x32   256  512  f44_pre    f24_pre    f44_pre
enc4.block.4   32x32   512  512  f44_pre    f44_pre    f44_pre
dec1.block.0   16x16   512 1024  f24_pre    f22        f24_pre
dec1.block.3   16x16  1024 1024  f24_pre    f24_pre    f24_pre
dec2.block.0   32x32  1024  512  f44_pre    f44_pre    f44_pre
dec2.block.3   32x32   512  512  f44_pre    f44_pre    f44_pre
dec3.block.0   64x64   512  256  f44_pre    f44_pre    f44_pre
dec3.block.3   64x64   256  256  f44_pre    f44_pre    f44_pre
dec4.block.0  128x128  256  128  f44_pre    f44_pre    f44_pre
dec4.block.3  128x128  128  128  f44_pre    f44_pre    f44_pre
last.0        256x256  128   64  f24        f44_pre    f24
last.3        256x256   64   64  f24_direct f24_direct f24
'''
CONFIG2_FP32_NO_FILTER_FOLD_BN = {'sums_by': {},
 'fold_src': {'enc2.block.4': 'enc2.block.1',
              'enc3.block.4': 'enc3.block.1',
              'enc4.block.4': 'enc4.block.1',
              'dec1.block.3': 'dec1.block.0',
              'dec2.block.3': 'dec2.block.0',
              'dec3.block.3': 'dec3.block.0',
              'dec4.block.3': 'dec4.block.0'},
 'fold_a': {},
 'pool_fold': {},
 'head_fold': []}

CASES = [
    (16, 256, 256, 'fp32', {}, CONFIG2_FP32, CONFIG2_FP32_BN),
    (16, 256, 256, 'bf16', {}, CONFIG2_BF16, CONFIG2_BF16_BN),
    (16, 256, 256, 'bf16x3', {}, CONFIG2_BF16X3, CONFIG2_BF16X3_BN),
    (32, 512, 512, 'bf16', {}, CONFIG5_BF16, CONFIG5_BF16_BN),
    (2, 512, 256, 'fp32', {}, REFERENCE_FP32, REFERENCE_FP32_BN),
    (16, 256, 256, 'fp32', {'WINOGRAD44': False}, CONFIG2_FP32_NO_F44, CONFIG2_FP32_NO_F44_BN),
    (16, 256, 256, 'fp32', {'FOLD_BN_INTO_FILTERS': False}, CONFIG2_FP32_NO_FILTER_FOLD, CONFIG2_FP32_NO_FILTER_FOLD_BN),
]


@pytest.mark.parametrize('B,H,W,dtype,switches,table,bn', CASES,
                         ids=['config2-fp32', 'config2-bf16', 'config2-bf16x3', 'config5-bf16', 'reference-fp32', 'config2-fp32-no-f44',
                              'config2-fp32-no-filter-fold'])
def test_plan_tables(B, H, W, dtype, switches, table, bn):
    from continual_learning_amd import plan as P, unet as U
    units = P.plan_net(U.stage_table(21, 3, 64), B, H, W, U._DTYPES[dtype][0], U.switches()._replace(**switches))
    got = [f"{u.name:13s} {u.h:3d}x{u.w:<3d} {u.cin_p:4d} {u.cout_p:4d}  {u.fwd:10s} {u.dgrad or '-':10s} {u.wgrad}" for u in units]
    assert got == table.strip('\n').split('\n')
    assert {u.name: u.sums_by for u in units if u.sums_by} == bn['sums_by']
    assert {u.name: u.fold_src for u in units if u.fold_src} == bn['fold_src']
    assert {u.name: u.fold_a for u in units if u.fold_a} == bn['fold_a']
    assert {u.name: u.pool_fold for u in units if u.pool_fold} == bn['pool_fold']
    assert [u.name for u in units if u.head_fold] == bn['head_fold']
    assert all(a in P.ALGOS for u in units for a in (u.fwd, u.wgrad) + ((u.dgrad,) if u.dgrad else ()))


def test_plan_switch_snapshot(monkeypatch):
    """The engine plans from the module's switches as they are when it is built (tests and tools/step_ab.py set them)."""
    from continual_learning_amd import plan as P, unet as U
    monkeypatch.setattr(U, 'WINOGRAD', False)
    units = P.plan_net(U.stage_table(21, 3, 64), 2, 64, 64, U._DTYPES['fp32'][0], U.switches())
    assert {u.fwd for u in units} == {'im2col', 'igemm'}
