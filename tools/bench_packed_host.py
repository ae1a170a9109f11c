#!/usr/bin/env python3
"""Host time of the smallest calls on the packed-byte path: `fh.state_counts()`,
`fh.state_series(...)` and `fh.read_packed(...)` on the sample VDIF and Mark 5B files,
opened on a device tensor.  The requests are a few frames, so the kernels take
microseconds and the wall clock around a call plus a synchronize is the host's work.

    python tools/bench_packed_host.py [--root TREE] [--against TREE] [--calls 400] [--label NAME]

`--root` names the tree whose `baseband_amd` is measured (default: this one).  With
`--against` the packages of both trees are loaded into the one process under names of
their own and take turns call by call, `--root`'s first: processes on one box differ by
more than two trees do, calls inside one process do not.  One JSON line, medians in
microseconds.
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name, root):
    """The package of the tree `root` under the module name `name` (its imports are relative)."""
    pkg = os.path.join(os.path.abspath(root), 'baseband_amd')
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def calls_of(package):
    import numpy as np
    import torch
    vdif, mark5b, _lib = (importlib.import_module(package.__name__ + m) for m in ('.vdif', '.mark5b', '._lib'))

    def image(name):
        return torch.from_numpy(np.fromfile(os.path.join(HERE, 'tests', 'golden', 'samples', name), np.uint8)).cuda()

    fv = vdif.open(image('sample.vdif'), 'rs', squeeze=False)
    fm = mark5b.open(image('sample.m5b'), 'rs', sample_rate=32e6, kday=56000, nchan=8, bps=2, squeeze=False)

    def read_packed(fh, coder, nthread, nchan, spf):     # one frame of the other sample file's geometry
        def call():
            fh.seek(0)
            return fh.read_packed(spf, coder, nthread, nchan, spf, 0)
        return call

    return {'vdif.state_counts': fv.state_counts,
            'vdif.state_series': lambda: fv.state_series(fv.samples_per_frame // 4),
            'vdif.read_packed': read_packed(fv, _lib.CODER_MARK5B, 1, 8, 5000),
            'm5b.state_counts': fm.state_counts,
            'm5b.state_series': lambda: fm.state_series(fm.samples_per_frame // 4),
            'm5b.read_packed': read_packed(fm, _lib.CODER_VDIF, 8, 1, 20000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--against', default=None)
    ap.add_argument('--calls', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--label', default=None)
    args = ap.parse_args()
    import torch
    roots = [args.root] + ([args.against] if args.against else [])
    trees = [calls_of(load('bb_tree{}'.format(k), root)) for k, root in enumerate(roots)]
    medians = {}
    for what in trees[0]:
        times = [[] for _ in trees]
        for calls in trees:
            for _ in range(args.warmup):
                calls[what]()
        torch.cuda.synchronize()
        for _ in range(args.calls):
            for calls, t in zip(trees, times):
                t0 = time.perf_counter()
                calls[what]()
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
        medians[what] = [round(statistics.median(t) * 1e6, 2) for t in times]
    print(json.dumps({'label': args.label or ' / '.join(roots), 'trees': roots, 'calls': args.calls, 'median_us': medians}))


if __name__ == '__main__':
    main()
