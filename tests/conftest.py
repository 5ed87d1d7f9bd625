import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu on the GPU box)')


def pytest_collection_modifyitems(config, items):
    # GPU tests are skipped (not failed) where no device exists, e.g. `pytest tests` in the build container.
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason='no GPU in this container')
    for it in items:
        if 'gpu' in it.keywords:
            it.add_marker(skip)


@pytest.fixture(autouse=True)
def _collect_garbage_between_gpu_tests(request):
    """Full-size tests hold tens of GB each; whatever a test leaves in reference cycles is collected before the next one."""
    yield
    if 'gpu' in request.keywords:
        import gc
        gc.collect()


class _JoinedArchive(dict):
    """The arrays of a golden archive stored in parts (<stem>.npz, <stem>.part2.npz, ...: oracle/gen_golden.save_golden keeps
    every committed file under 1 MiB), with the `.files` list of an NpzFile."""
    @property
    def files(self):
        return list(self)


@pytest.fixture(scope='session')
def golden():
    def load(name):
        path = os.path.join(GOLDEN, name)
        stem = path[:-len('.npz')]
        if not os.path.exists(f'{stem}.part2.npz'):
            return np.load(path, allow_pickle=False)
        joined, i = _JoinedArchive(), 1
        while os.path.exists(part := path if i == 1 else f'{stem}.part{i}.npz'):
            with np.load(part, allow_pickle=False) as z:
                joined.update((k, z[k]) for k in z.files)
            i += 1
        return joined
    return load


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
