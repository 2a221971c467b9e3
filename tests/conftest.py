import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


class Fixture:
    """npz fixture with torch access: fx['name'] -> tensor, fx.sub('prefix.') -> dict.  A fixture larger than a committed file
    may be stored in parts (name.npz, name.part2.npz, ...: tests/golden/make_golden.py), read here as one, keys in order."""

    def __init__(self, name):
        paths = [os.path.join(GOLDEN, name + ".npz")]
        paths += sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")), key=lambda p: int(p.split(".part")[-1][:-4]))
        parts = [np.load(p, allow_pickle=False) for p in paths]
        self._files = [k for z in parts for k in z.files]
        self._part = {k: z for z in parts for k in z.files}

    def __contains__(self, k):
        return k in self._part

    def __getitem__(self, k):
        a = self._part[k][k]
        if a.dtype.kind in "US":
            return a
        if a.dtype == np.uint64:          # exact integer checksums
            return int(a) if a.ndim == 0 else [int(v) for v in a.reshape(-1)]
        return torch.from_numpy(np.array(a))

    def keys(self):
        return list(self._files)

    def sub(self, prefix):
        return {k[len(prefix):]: self[k] for k in self._files if k.startswith(prefix)}


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = Fixture(name)
        return cache[name]

    return load


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())
