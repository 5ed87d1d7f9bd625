"""Exemplar replay for the task step (build-defined, parity unpinned: the reference has no continual-learning code).

Rehearsal: a small on-device memory of exemplars from finished tasks, mixed into every batch of the new task.  The store keeps the images
as uint8 (a quarter of fp32's bytes; exact for images that came from the uint8 data path, within 1/255 otherwise) or fp32 and the labels
as uint8; filling is class-balanced reservoir sampling decided on the host (``assign_slots``) from per-image class counts; the step's batch
of B current + R replayed images, decoded and flipped, is ONE launch.

    mem = ReplayMemory(num_classes=21, image_shape=(3, 256, 256))
    mem.add_task(classes=(1, 11), capacity=100)
    mem.fill(task1_loader, 'cuda')                        # or observe(images, labels) per batch, then finish()
    x, y = mem.mix(images, labels, 4)                     # rows [0, B) are the inputs, rows [B, B + 4) exemplars

All three device passes run on libclamd's kernels (clamd_class_pixel_counts, clamd_replay_store, clamd_replay_mix; include/clamd.h states
the encodings).  Data parallelism: each rank keeps its own memory, filled from its own shard of the data and sampled with ``seed + rank``
(Trainer.begin_task2 passes that seed); the gradients are averaged as always and no collective is added.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr

STORAGES = ('uint8', 'fp32')


def _hbm(nbytes, name, *args):
    from . import unet as U
    U._hbm('replay', nbytes, name, *args)


def _check_labels(labels):
    if not labels.is_cuda:
        raise RuntimeError('continual-learning_amd exemplar replay runs only on GPU tensors: there is no CPU fallback')
    if labels.dtype != torch.int64 or labels.dim() != 3:
        raise TypeError('labels must be an int64 [B, H, W] tensor (datasets/voc.py:72)')


def class_pixel_counts(labels, num_classes, ignore_index=-100):
    """-> device int32 [B, num_classes]: counts[b, k] = pixels of image b with label k (clamd_class_pixel_counts).  Labels equal to
    ignore_index are skipped; other labels outside [0, num_classes) are skipped and counted in ``.bad_labels`` of the returned tensor (device
    int32 [1]; int(...) synchronises), as the criteria keep theirs."""
    if not 1 <= int(num_classes) <= 255:
        raise ValueError('num_classes must be in [1, 255]')
    _check_labels(labels)
    B, H, W = labels.shape
    y = labels if labels.is_contiguous() else labels.contiguous()      # a view at a storage offset stays as it is: the one-label path
    counts = torch.empty(B, int(num_classes), dtype=torch.int32, device=labels.device)
    bad = torch.zeros(1, dtype=torch.int32, device=labels.device)
    _hbm(B * H * W * 8, 'clamd_class_pixel_counts', ptr(y), ptr(counts), ptr(bad), B, int(num_classes), H, W, int(ignore_index), _lib.stream_ptr())
    counts.bad_labels = bad
    return counts


class Segment:
    """The slots of one finished task and the policy's counters: classes [lo, hi), ``capacity`` slots from ``base`` on -- q = capacity // n
    per class in class order (class c's start at base + (c - lo) * q), then g = capacity - q * n of a general reservoir.  ``seen[c - lo]`` /
    ``seen_general``: how many images each reservoir has been offered.  ``rng``: the numpy Generator Algorithm R draws from."""

    def __init__(self, lo, hi, capacity, min_pixels=1, base=0, rng=None):
        lo, hi, capacity, min_pixels = int(lo), int(hi), int(capacity), int(min_pixels)
        n = hi - lo
        if lo < 1:
            raise ValueError('classes: lo must be >= 1 (class 0 is the background of every task)')
        if n < 1:
            raise ValueError('classes: hi must be above lo')
        if capacity < n:
            raise ValueError(f'capacity {capacity} is below the number of classes {n}: every class owns at least one slot')
        if min_pixels < 1:
            raise ValueError('min_pixels must be >= 1')
        self.lo, self.hi, self.capacity, self.min_pixels, self.base = lo, hi, capacity, min_pixels, int(base)
        self.q = capacity // n
        self.g = capacity - self.q * n
        self.seen = np.zeros(n, dtype=np.int64)
        self.seen_general = 0
        self.rng = rng if rng is not None else np.random.Generator(np.random.PCG64(0))

    def class_base(self, c):
        return self.base + (c - self.lo) * self.q

    @property
    def general_base(self):
        return self.base + (self.hi - self.lo) * self.q

    def filled_slots(self):
        """Occupied slots, ascending: a reservoir of size s that was offered t images holds min(t, s)."""
        out = []
        for c in range(self.lo, self.hi):
            out.extend(range(self.class_base(c), self.class_base(c) + min(int(self.seen[c - self.lo]), self.q)))
        out.extend(range(self.general_base, self.general_base + min(self.seen_general, self.g)))
        return out

    def state_dict(self):
        return dict(lo=self.lo, hi=self.hi, capacity=self.capacity, min_pixels=self.min_pixels, base=self.base,
                    seen=[int(v) for v in self.seen], seen_general=int(self.seen_general))

    @classmethod
    def from_state(cls, st, rng):
        seg = cls(st['lo'], st['hi'], st['capacity'], st['min_pixels'], st['base'], rng)
        seg.seen[:] = st['seen']
        seg.seen_general = int(st['seen_general'])
        return seg


def _algorithm_r(t, size, rng):
    """Vitter's Algorithm R for the t-th (0-based) image offered to a reservoir of `size` slots -> offset in [0, size) or None (dropped).
    One draw per image that arrives at a full reservoir, none otherwise."""
    if t < size:
        return t
    if size == 0:
        return None
    j = int(rng.integers(0, t + 1))
    return j if j < size else None


def assign_slots(counts_rows, seg):
    """The class-balanced reservoir policy, a pure host function: counts_rows [n, K] (per-image class pixel counts, stream order), seg a
    Segment whose counters and rng advance.  -> [(row, slot)] of the images to store, in stream order (a later pair with the same slot
    replaces an earlier one).  Per image: present = the segment's classes with at least min_pixels pixels; non-empty: the image is
    offered to exactly one class, the one whose reservoir has been offered the fewest images (ties: the lowest class), by Algorithm R on
    that class's q slots; empty: Algorithm R on the general reservoir (dropped when it has no slots).  An image is never stored twice."""
    counts_rows = np.asarray(counts_rows)
    if counts_rows.ndim != 2 or counts_rows.shape[1] < seg.hi:
        raise ValueError(f'counts_rows must be [n, K >= {seg.hi}]')
    out = []
    for row in range(counts_rows.shape[0]):
        present = [c for c in range(seg.lo, seg.hi) if int(counts_rows[row, c]) >= seg.min_pixels]
        if present:
            c = min(present, key=lambda k: (int(seg.seen[k - seg.lo]), k))
            t = int(seg.seen[c - seg.lo])
            seg.seen[c - seg.lo] = t + 1
            off, first = _algorithm_r(t, seg.q, seg.rng), seg.class_base(c)
        else:
            t = seg.seen_general
            seg.seen_general = t + 1
            off, first = _algorithm_r(t, seg.g, seg.rng), seg.general_base
        if off is not None:
            out.append((row, first + off))
    return out


def _last_per_slot(pairs):
    """One launch writes each slot once: of several images assigned to one slot the last one is what the store would end up holding."""
    last = {}
    for row, slot in pairs:
        last[slot] = row
    return sorted((row, slot) for slot, row in last.items())


class ReplayMemory:
    """The exemplar store of every finished task and its sampler.  ``images`` [capacity, C, H, W] uint8 or float32 and ``labels``
    [capacity, H, W] uint8 live on the device of the first batch offered; ``filled`` is the device int64 list of occupied slots (rebuilt
    by finish()); ``bad_labels`` / ``bad_slots`` are device int32 [1] counters (labels that were neither ignore_index nor a class when
    stored; slots outside the store met by mix, a guard that stays 0)."""

    def __init__(self, num_classes, image_shape, storage='uint8', ignore_index=-100, flip=True, seed=0):
        if not 1 <= int(num_classes) <= 255:
            raise ValueError('num_classes must be in [1, 255] (a stored label is one byte and 255 is the ignore value)')
        if storage not in STORAGES:
            raise ValueError(f'storage must be one of {STORAGES}')
        if len(image_shape) != 3 or min(int(v) for v in image_shape) < 1:
            raise ValueError('image_shape must be (C, H, W)')
        self.num_classes, self.image_shape = int(num_classes), tuple(int(v) for v in image_shape)
        self.storage, self.ignore_index, self.flip, self.seed = storage, int(ignore_index), bool(flip), int(seed)
        self.segments = []
        self.open = None                      # the Segment being filled, between add_task() and finish()
        self.rng = np.random.Generator(np.random.PCG64(self.seed))
        self.gen = None                       # device torch.Generator of mix(), created with the store
        self._gen_state = None                # a loaded generator state waiting for the device
        self.images = self.labels = self.filled = None
        self.n_filled = 0
        self.bad_labels = self.bad_slots = None

    @property
    def capacity(self):
        return sum(s.capacity for s in self.segments)

    def add_task(self, classes, capacity, min_pixels=1):
        """Appends a segment of `capacity` slots for a finished task whose foreground classes are [lo, hi) and opens it for observe()."""
        if self.open is not None:
            raise RuntimeError('ReplayMemory.add_task: the previous segment is still open (finish() first)')
        lo, hi = classes
        if int(hi) > self.num_classes:
            raise ValueError(f'classes [{lo}, {hi}) exceed num_classes {self.num_classes}')
        seg = Segment(lo, hi, capacity, min_pixels, base=self.capacity, rng=self.rng)
        self.segments.append(seg)
        self.open = seg
        return self

    def _ensure_store(self, device):
        C, H, W = self.image_shape
        if self.gen is None:
            self.gen = torch.Generator(device=device)
            self.gen.manual_seed(self.seed)
            if self._gen_state is not None:
                self.gen.set_state(self._gen_state)
                self._gen_state = None
            self.bad_labels = torch.zeros(1, dtype=torch.int32, device=device)
            self.bad_slots = torch.zeros(1, dtype=torch.int32, device=device)
        have = 0 if self.images is None else self.images.shape[0]
        if have < self.capacity:      # once per task: the earlier segments move into the grown store
            images = torch.zeros(self.capacity, C, H, W, dtype=torch.uint8 if self.storage == 'uint8' else torch.float32, device=device)
            labels = torch.full((self.capacity, H, W), 255, dtype=torch.uint8, device=device)
            if have:
                images[:have] = self.images
                labels[:have] = self.labels
            self.images, self.labels = images, labels

    def _check_batch(self, images, labels):
        _check_labels(labels)
        if not images.is_cuda or images.dtype != torch.float32:
            raise TypeError('images must be a float32 GPU tensor')
        if images.dim() != 4 or tuple(images.shape[1:]) != self.image_shape or tuple(labels.shape) != (images.shape[0],) + self.image_shape[1:]:
            raise ValueError(f'expected images [B, {self.image_shape}] and labels [B, H, W], got {tuple(images.shape)} and {tuple(labels.shape)}')
        return (images if images.is_contiguous() else images.contiguous()), (labels if labels.is_contiguous() else labels.contiguous())

    def observe(self, images, labels):
        """Offers one batch to the open segment: the count kernel, the [B, K] counts copied to the host -- a SYNCHRONISATION; filling
        happens once per task and is not the step --, the policy on the host, then one clamd_replay_store for the accepted images.
        -> the (row, slot) pairs that were stored."""
        if self.open is None:
            raise RuntimeError('ReplayMemory.observe: no open segment (add_task() first)')
        x, y = self._check_batch(images, labels)
        self._ensure_store(x.device)
        counts = class_pixel_counts(y, self.num_classes, self.ignore_index).cpu().numpy()
        pairs = _last_per_slot(assign_slots(counts, self.open))
        if pairs:
            self.store(x, y, [p[0] for p in pairs], [p[1] for p in pairs])
        return pairs

    def store(self, images, labels, src, slots):
        """Batch images src[i] -> slots[i] in one launch (clamd_replay_store); src and slots are host lists, checked here."""
        x, y = self._check_batch(images, labels)
        self._ensure_store(x.device)
        B, (C, H, W), cap, n = x.shape[0], self.image_shape, self.images.shape[0], len(src)
        if n == 0:
            return
        if len(slots) != n or len(set(slots)) != n:
            raise ValueError('store: one distinct slot per image')
        if min(src) < 0 or max(src) >= B or min(slots) < 0 or max(slots) >= cap:
            raise ValueError(f'store: src must lie in [0, {B}) and slots in [0, {cap})')
        idx = torch.tensor([list(src), list(slots)], dtype=torch.int32).to(x.device)
        px = 1 if self.storage == 'uint8' else 4
        # algorithmic bytes: the image and its labels read, the slot written
        _hbm(n * H * W * (C * (4 + px) + 9), 'clamd_replay_store', ptr(x), ptr(y), ptr(idx[0]), ptr(idx[1]), n, ptr(self.images),
             ptr(self.labels), int(self.storage == 'fp32'), cap, ptr(self.bad_labels), B, C, H, W, self.num_classes, self.ignore_index,
             _lib.stream_ptr())

    def finish(self):
        """Closes the open segment and rebuilds ``filled`` over all segments."""
        self.open = None
        occupied = [s for seg in self.segments for s in seg.filled_slots()]
        self.n_filled = len(occupied)
        if self.images is not None:
            self.filled = torch.tensor(occupied, dtype=torch.int64).to(self.images.device)
        return self

    def fill(self, loader, device, max_batches=None):
        """observe() over a loader of (images, labels) -- the FINISHED task's data --, then finish()."""
        for i, (images, masks) in enumerate(loader):
            if max_batches is not None and i >= max_batches:
                break
            self.observe(images.to(device, non_blocking=True), masks.to(device, non_blocking=True))
        return self.finish()

    def draw(self, R):
        """-> (slots int64 [R], flips int32 [R]) on the device from the device generator: filled[randint(len(filled))] and randint(4) (zeros
        with flip=False, no draw).  No host synchronisation."""
        dev = self.filled.device
        slots = self.filled[torch.randint(self.n_filled, (R,), generator=self.gen, device=dev)]
        if self.flip:
            flips = torch.randint(4, (R,), generator=self.gen, device=dev, dtype=torch.int32)
        else:
            flips = torch.zeros(R, dtype=torch.int32, device=dev)
        return slots, flips

    def _launch(self, x, y, B, slots, flips):
        (C, H, W), R = self.image_shape, slots.shape[0]
        dev = self.images.device
        out_x = torch.empty(B + R, C, H, W, dtype=torch.float32, device=dev)
        out_y = torch.empty(B + R, H, W, dtype=torch.int64, device=dev)
        px = 1 if self.storage == 'uint8' else 4
        # algorithmic bytes: the current batch read and written, the exemplars read from the store and written decoded
        _hbm(H * W * (B * (8 * C + 16) + R * (C * (px + 4) + 9)), 'clamd_replay_mix', ptr(x), ptr(y), B, ptr(self.images), ptr(self.labels),
             int(self.storage == 'fp32'), self.images.shape[0], ptr(slots), ptr(flips), R, ptr(out_x), ptr(out_y), ptr(self.bad_slots),
             C, H, W, self.ignore_index, _lib.stream_ptr())
        return out_x, out_y

    def mix(self, images, labels, R):
        """-> (images', labels') of B + R rows in one launch (clamd_replay_mix): rows [0, B) bit-copies of the inputs, rows [B, B + R)
        exemplars from draw(R), decoded and flipped.  R == 0 or an empty memory: the inputs themselves, no launch.  No host
        synchronisation."""
        R = int(R)
        if R < 0:
            raise ValueError('R must be >= 0')
        if R == 0 or self.n_filled == 0 or self.filled is None:
            return images, labels
        x, y = self._check_batch(images, labels)
        if x.device != self.images.device:
            raise ValueError('the batch and the memory are on different devices')
        slots, flips = self.draw(R)
        return self._launch(x, y, x.shape[0], slots, flips)

    def gather(self, slots, flips=None):
        """The B = 0 form, for inspection and tests: exemplars `slots` (a list or an int64 tensor) with flip codes `flips` (None: none)."""
        if self.images is None:
            raise RuntimeError('ReplayMemory.gather: nothing has been stored')
        dev = self.images.device
        slots = torch.as_tensor(slots, dtype=torch.int64).to(dev).contiguous()
        if slots.dim() != 1 or slots.numel() == 0:
            raise ValueError('slots must be a non-empty 1-D list')
        if flips is not None:
            flips = torch.as_tensor(flips, dtype=torch.int32).to(dev).contiguous()
            if flips.shape != slots.shape:
                raise ValueError('one flip code per slot')
        return self._launch(None, None, 0, slots, flips)

    def state_dict(self):
        """The stores, the segments with the policy's counters, and both RNG states (the host numpy one of the policy, the device torch
        one of mix)."""
        gen_state = self.gen.get_state() if self.gen is not None else self._gen_state
        return dict(num_classes=self.num_classes, image_shape=self.image_shape, storage=self.storage, ignore_index=self.ignore_index,
                    flip=self.flip, seed=self.seed, images=self.images, labels=self.labels,
                    segments=[s.state_dict() for s in self.segments], open=self.open is not None,
                    policy_rng=self.rng.bit_generator.state, mix_rng=gen_state)

    def load_state_dict(self, state, device=None):
        """Restores state_dict()'s result; the stores go to `device` (default: where the state's tensors are; a CPU state, as a checkpoint
        holds, needs one)."""
        for k in ('num_classes', 'storage', 'ignore_index'):
            if state[k] != getattr(self, k):
                raise ValueError(f'replay state has {k}={state[k]!r}, this memory {getattr(self, k)!r}')
        if tuple(state['image_shape']) != self.image_shape:
            raise ValueError(f'replay state has image_shape={tuple(state["image_shape"])}, this memory {self.image_shape}')
        self.flip, self.seed = bool(state['flip']), int(state['seed'])
        self.rng = np.random.Generator(np.random.PCG64(self.seed))
        self.rng.bit_generator.state = state['policy_rng']
        self.segments = [Segment.from_state(st, self.rng) for st in state['segments']]
        self.open = self.segments[-1] if state['open'] else None
        self.images = self.labels = self.filled = self.gen = None
        self.n_filled = 0
        self._gen_state = state['mix_rng']
        if state['images'] is not None:
            dev = torch.device(device) if device is not None else state['images'].device
            if dev.type != 'cuda':
                raise RuntimeError('continual-learning_amd exemplar replay keeps its store on the GPU: pass device=')
            self._ensure_store(dev)
            self.images.copy_(state['images'])
            self.labels.copy_(state['labels'])
        occupied = self.open
        self.finish()
        self.open = occupied
        return self
