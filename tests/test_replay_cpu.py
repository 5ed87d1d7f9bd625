"""CPU: exemplar replay (build-defined: the reference has no continual-learning code, parity unpinned) -- the three entry points in the
header, the ctypes table and the library; the class-balanced reservoir policy ``replay.assign_slots`` against an independent restatement
of its rule and against its invariants; the uint8 quantisation formulas of include/clamd.h restated in numpy float32; the argument errors,
all raised before any library call."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import continual_learning_amd as C
from continual_learning_amd import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_DATA = 5           # synth.labels seed of the policy's stream: 40 images of 32 x 32 in 16 x 16 cells, 6 classes
LO, HI, M = 1, 4, 7     # classes [1, 4), 7 slots: q = 2 per class, g = 1 general


# ------------------------------------------------------------------------------------------------------------------------- entry points
@pytest.mark.parametrize('name,nargs', [('clamd_class_pixel_counts', 9), ('clamd_replay_store', 17), ('clamd_replay_mix', 18)])
def test_entry_points_in_header_ctypes_table_and_library(name, nargs):
    header = open(os.path.join(ROOT, 'include', 'clamd.h')).read()
    m = re.search(r'int\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
    assert m, 'prototype missing from include/clamd.h'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert len(args) == len(C._lib.SIGNATURES[name][1]) == nargs
    assert args[-1] == 'void* stream'
    out = subprocess.run(['nm', '-D', '--defined-only', C._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\sT\s+' + name + r'\s*$', out, re.M), 'libclamd.so does not export the entry point'
    assert hasattr(C._lib.load(), name)


def test_package_exports():
    assert C.ReplayMemory is replay.ReplayMemory and C.class_pixel_counts is replay.class_pixel_counts and C.replay is replay
    assert 'replay.hip' in open(os.path.join(ROOT, 'continual-learning_amd', 'build.py')).read()


# ------------------------------------------------------------------------------------------------------------------------------- policy
@pytest.fixture(scope='module')
def counts():
    lab = C.synth.labels(SEED_DATA, 40, 32, 32, 6)
    return np.stack([np.bincount(im.ravel(), minlength=6) for im in lab])


def restated_policy(counts, lo, hi, capacity, min_pixels, seed):
    """The rule of the issue, written out again: -> (pairs [(row, slot)], trace [(row, reservoir, offered before, size, slot or None)]).
    reservoir: a class, or None for the general one."""
    n = hi - lo
    q = capacity // n
    g = capacity - q * n
    rng = np.random.Generator(np.random.PCG64(seed))
    offered = {c: 0 for c in range(lo, hi)}
    offered[None] = 0
    first = {c: (c - lo) * q for c in range(lo, hi)}
    first[None] = n * q
    pairs, trace = [], []
    for row in range(len(counts)):
        present = [c for c in range(lo, hi) if counts[row][c] >= min_pixels]
        res = sorted(present, key=lambda c: (offered[c], c))[0] if present else None
        size = q if present else g
        t = offered[res]
        offered[res] += 1
        slot = None
        if t < size:
            slot = first[res] + t
        elif size > 0:
            j = int(rng.integers(0, t + 1))
            if j < size:
                slot = first[res] + j
        trace.append((row, res, t, size, slot))
        if slot is not None:
            pairs.append((row, slot))
    return pairs, trace


def run_policy(counts, min_pixels=1, seed=0, chunks=(40,)):
    seg = replay.Segment(LO, HI, M, min_pixels, base=0, rng=np.random.Generator(np.random.PCG64(seed)))
    pairs, at = [], 0
    for n in chunks:      # the stream arrives in batches: the rows of a batch count from 0
        pairs += [(at + r, s) for r, s in replay.assign_slots(counts[at:at + n], seg)]
        at += n
    return pairs, seg


def test_policy_equals_the_restatement(counts):
    want, trace = restated_policy(counts, LO, HI, M, 1, 0)
    got, seg = run_policy(counts)
    assert got == want
    assert (seg.q, seg.g) == (2, 1)
    # the stream exercises every branch: a class reservoir past its size (Algorithm R draws), the general reservoir, a drop and a replacement
    assert any(res is not None and t >= size for _, res, t, size, _ in trace)
    assert any(res is None for _, res, _, _, _ in trace)
    assert any(slot is None for *_, slot in trace) and any(t >= size and slot is not None for _, _, t, size, slot in trace)
    # the same stream in batches of 7, 1, 12, 20: the counters and the generator carry over
    assert run_policy(counts, chunks=(7, 1, 12, 20))[0] == want
    assert seg.filled_slots() == list(range(M))


def test_policy_with_min_pixels_above_a_class_largest_blob(counts):
    mp = int(counts[:, 3].max()) + 1            # class 3 is never present; the other classes only where they cover more than that
    want, trace = restated_policy(counts, LO, HI, M, mp, 0)
    got, seg = run_policy(counts, min_pixels=mp)
    assert got == want
    assert all(res != 3 for _, res, _, _, _ in trace) and int(seg.seen[3 - LO]) == 0
    assert not set(seg.filled_slots()) & {4, 5}, 'class 3 owns slots 4 and 5: they stay empty'
    assert got != run_policy(counts)[0]


@pytest.mark.parametrize('min_pixels', [1, 300])
def test_policy_invariants(counts, min_pixels):
    pairs, seg = run_policy(counts, min_pixels=min_pixels)
    rows = [r for r, _ in pairs]
    assert len(rows) == len(set(rows)), 'an image was stored twice'
    held = {}
    for r, s in pairs:
        held[s] = r
    assert len(set(held.values())) == len(held)
    for s, r in held.items():      # a class's slots hold only images that contain it with at least min_pixels pixels
        assert 0 <= s < M
        if s < 3 * seg.q:
            c = LO + s // seg.q
            assert counts[r][c] >= min_pixels, (s, r, c)
        else:
            assert all(counts[r][c] < min_pixels for c in range(LO, HI)), (s, r)
    # no offered image is dropped while its reservoir has room
    _, trace = restated_policy(counts, LO, HI, M, min_pixels, 0)
    stored = dict(pairs)
    for row, res, t, size, _ in trace:
        if t < size:
            assert row in stored and stored[row] == (3 * seg.q if res is None else (res - LO) * seg.q) + t
    # the same seed gives the same assignment, another seed another one
    assert run_policy(counts, min_pixels=min_pixels)[0] == pairs
    assert run_policy(counts, min_pixels=min_pixels, seed=1)[0] != pairs


def test_one_launch_writes_each_slot_once():
    assert replay._last_per_slot([(0, 4), (1, 2), (2, 4), (3, 0)]) == [(1, 2), (2, 4), (3, 0)]


def test_state_dict_carries_the_policy(counts):
    a = C.ReplayMemory(6, (3, 32, 32), seed=3).add_task((LO, HI), M)
    first = replay.assign_slots(counts[:25], a.open)
    st = a.state_dict()
    assert st['images'] is None and st['open'] and st['segments'][0]['seen'] == [int(v) for v in a.open.seen]
    b = C.ReplayMemory(6, (3, 32, 32), seed=99).load_state_dict(st)
    assert b.seed == 3 and b.open is b.segments[-1]
    assert replay.assign_slots(counts[25:], b.open) == replay.assign_slots(counts[25:], a.open)
    assert first == restated_policy(counts[:25], LO, HI, M, 1, 3)[0]
    with pytest.raises(ValueError, match='storage'):
        C.ReplayMemory(6, (3, 32, 32), storage='fp32').load_state_dict(st)


# ------------------------------------------------------------------------------------------------------------------------- quantisation
def encode(x):
    """include/clamd.h: u = clamp(rintf((x * 0.5f + 0.5f) * 255.f), 0, 255), every operation in float32."""
    x = np.asarray(x, dtype=np.float32)
    t = np.rint((x * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0))
    assert t.dtype == np.float32
    return np.clip(t, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def decode(u):
    """voc_prepare_kernel's arithmetic: v = (float)u / 255.f; x = (v - 0.5f) / 0.5f."""
    v = np.asarray(u).astype(np.float32) / np.float32(255.0)
    x = (v - np.float32(0.5)) / np.float32(0.5)
    assert x.dtype == np.float32
    return x


def test_every_byte_survives_decode_encode_decode():
    u = np.arange(256, dtype=np.uint8)
    x = decode(u)
    assert np.array_equal(encode(x), u)
    assert np.array_equal(decode(encode(x)).view(np.uint32), x.view(np.uint32))
    assert x[0] == -1.0 and x[255] == 1.0
    assert np.array_equal(encode(np.float32([-3.0, 3.0, -1.0, 1.0])), np.uint8([0, 255, 0, 255]))


def test_quantisation_error_is_half_a_step():
    x = C.synth.images(1234, 2, 3, 32, 48)
    err = float(np.abs(decode(encode(x)).astype(np.float64) - x.astype(np.float64)).max())
    print(f'max |decode(encode(x)) - x| = {err:.7f} against 1/255 = {1 / 255:.7f}')
    # a step of u is 2/255 in x units, rounding to nearest leaves half of it; 1e-6: a few float32 roundings at |x| <= 1
    assert err <= 1 / 255 + 1e-6


# --------------------------------------------------------------------------------------------------------------------- argument errors
@pytest.fixture
def no_library_call(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a library call was made')
    monkeypatch.setattr(C.unet, '_hbm', refuse)
    monkeypatch.setattr(C._lib, 'call', refuse)


def test_argument_errors_come_before_any_library_call(no_library_call):
    mem = C.ReplayMemory(6, (3, 32, 32))
    with pytest.raises(ValueError, match='capacity'):
        mem.add_task((1, 4), 2)                                # M < n
    with pytest.raises(ValueError, match='lo must be >= 1'):
        mem.add_task((0, 4), 8)
    with pytest.raises(ValueError, match='hi must be above lo'):
        mem.add_task((3, 3), 8)
    with pytest.raises(ValueError, match='exceed num_classes'):
        mem.add_task((1, 7), 8)
    assert mem.segments == [] and mem.open is None
    with pytest.raises(ValueError, match='num_classes'):
        C.ReplayMemory(256, (3, 32, 32))
    with pytest.raises(ValueError, match='storage'):
        C.ReplayMemory(6, (3, 32, 32), storage='bf16')
    with pytest.raises(ValueError, match='image_shape'):
        C.ReplayMemory(6, (32, 32))
    x, y = torch.zeros(2, 3, 32, 32), torch.zeros(2, 32, 32, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='add_task'):
        mem.observe(x, y)
    mem.add_task((1, 4), 8)
    with pytest.raises(RuntimeError, match='still open'):
        mem.add_task((4, 6), 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mem.observe(x, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        C.class_pixel_counts(y, 6)
    with pytest.raises(ValueError, match='num_classes'):
        C.class_pixel_counts(y, 256)
    # an empty memory hands the batch back untouched, R == 0 too
    assert mem.mix(x, y, 2)[0] is x and mem.mix(x, y, 0)[1] is y


def test_begin_task2_refuses_replay_without_a_replay_batch(no_library_call):
    tr = C.Trainer([], C.default_config(num_classes=5, conv_dim=4), device='cpu')
    with pytest.raises(ValueError, match='replay_batch'):
        tr.begin_task2(5, replay=4, replay_batch=0)
    with pytest.raises(ValueError, match='>= 0'):
        tr.begin_task2(5, replay=-1)
    assert tr.old_model is None and tr.replay is None and tr.replay_batch == 0      # refused before anything was switched on
