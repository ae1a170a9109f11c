"""``bench.py --dump-outputs DIR``: what the timed path computed in its last
step, written as ``DIR/<name>.npy`` (float32 or float64, nothing else in DIR)
so that two builds can be compared output for output.

An array that fits its share of the byte budget is written whole; a larger one
is written as a stratified sample of its flattened elements: the array is cut
into ``k`` equal strata and one element is taken from each, at a position drawn
from a generator seeded by a fixed seed.  The positions depend only on the
array's size, the budget and the seed, so the same arguments sample the same
elements in every run and every region of the output is represented."""
import os

import numpy as np
import torch

DUMP_BUDGET_BYTES = 60 * 2 ** 20        # all files of one run together (below 64 MB)
DUMP_SEED = 20240601


def sample_positions(n, k, seed=DUMP_SEED):
    """``k`` sorted positions in ``[0, n)``, one per stratum of ``ceil(n / k)``
    elements (int64 CPU tensor); ``arange(n)`` when ``k >= n``."""
    if k >= n:
        return torch.arange(n, dtype=torch.int64)
    stride = -(-n // k)
    k = -(-n // stride)                                 # strata that start inside the array
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    pos = torch.arange(k, dtype=torch.int64) * stride \
        + torch.randint(0, stride, (k,), generator=g, dtype=torch.int64)
    return pos.clamp_(max=n - 1)


def dump_outputs(dirpath, arrays, budget=DUMP_BUDGET_BYTES, seed=DUMP_SEED):
    """Write ``arrays`` ({name: (tensor, numpy float dtype)}) into ``dirpath``.
    The budget is split evenly between the arrays; each is converted to its
    float dtype on the host (float64 holds every int32 and every int64 below
    2^53 exactly).  Returns {name: what was written}."""
    os.makedirs(dirpath, exist_ok=True)
    share = budget // max(1, len(arrays))
    written = {}
    for name, (t, dtype) in arrays.items():
        dtype = np.dtype(dtype)
        assert dtype in (np.float32, np.float64), dtype
        flat = t.reshape(-1)
        n = flat.numel()
        k = max(1, share // dtype.itemsize)
        if k >= n:
            host = t.cpu().numpy()
            what = "whole"
        else:
            pos = sample_positions(n, k, seed)
            host = flat[pos.to(flat.device)].cpu().numpy()
            what = "stratified sample of {} of {} elements, one per {} (seed {})".format(
                pos.numel(), n, -(-n // k), seed)
        host = host.astype(dtype, copy=False)
        np.save(os.path.join(dirpath, name + '.npy'), host)
        written[name] = "{} {} of {} {}: {}".format(
            dtype.name, list(host.shape), str(t.dtype).replace('torch.', ''), list(t.shape), what)
    return written
