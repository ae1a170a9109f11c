#!/usr/bin/env python
"""Kernel time of the sampler statistics (bb_count_states, k_states.h) against two
yardsticks, on one GPU.

For every row three launches are timed, taking turns inside every repetition, on the
same 1 GiB of frames at a fixed stride:
  (s) bb_count_states: every payload byte read once, a few dozen integers added,
  (t) bb_touch of the window: the library's read-once launch, the ceiling of any
      read-only kernel,
  (d) the float32 bb_decode_frames launch of the same frames: what a user pays today
      before any counting starts (17 times the bytes).
HIP events around the launches on the launching stream; two warm-up rounds; every
launch takes the NEXT 1 GiB window of a larger image, so that no input is still in the
256 MiB memory-side cache.  Reported: the median time, the window's bytes over that
time for (s) and (t), and the two relations the design answers to: (s) below (d),
(s) no more than 1.3 times (t).

    python tools/bench_states.py [--reps 7] [--windows 3] > profiles/states.log
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOW = 1 << 30
AIM = 1.3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Row:
    def __init__(self, name, coder, bps, chunk, frame, hdr, zeros=False):
        self.name, self.coder, self.bps, self.chunk, self.frame, self.hdr = name, coder, bps, chunk, frame, hdr
        self.zeros = zeros
        self.pn = frame - hdr
        self.nf = WINDOW // frame
        self.nelem = self.nf * self.pn * 8 // bps


def run_row(row, image, reps):
    import baseband_amd
    from baseband_amd import kernels, _lib
    dev = image.device
    nwin = image.numel() // WINDOW
    out = baseband_amd.empty_output(row.nelem, torch.float32, dev)
    counts = torch.zeros((1, row.chunk, 1 << row.bps), dtype=torch.int64, device=dev)
    turn = [0]

    def window():
        k = turn[0] % nwin
        return image[k * WINDOW:(k + 1) * WINDOW]

    def s():
        kernels.count_states(window(), row.nf, row.pn, row.bps, row.chunk, src0=row.hdr, src_stride=row.frame,
                             counts=counts)

    def t():
        w = window()
        _lib.check(_lib.lib.bb_touch(ctypes.c_void_p(w.data_ptr()), row.nf * row.frame, kernels._stream(w)), 'bb_touch')

    def d():
        kernels.decode_frames(window(), row.nf, row.pn, row.coder, row.bps, chunk=row.chunk, src0=row.hdr,
                              src_stride=row.frame, out=out)

    ts = {'s': [], 't': [], 'd': []}
    for r in range(reps + 2):
        for key, fn in (('s', s), ('t', t), ('d', d)):
            turn[0] += 1
            ms = timed(fn)
            if r >= 2:
                ts[key].append(ms)
    decode_kernel = _lib.last_kernel()
    # what was counted: every code of every launch, once
    launches = reps + 2
    total = int(counts.sum())
    res = {'row': row.name, 'frames': row.nf, 'frame_nbytes': row.frame, 'bps': row.bps, 'chunk': row.chunk,
           'window_GB': round(row.nf * row.frame / 1e9, 4), 'windows': nwin, 'decode_kernel': decode_kernel,
           'codes_counted_ok': total == launches * row.nelem}
    for key in 'std':
        ms = float(np.median(ts[key]))
        res['ms_' + key] = round(ms, 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
    res['GBs_s'] = round(row.nf * row.frame / res['ms_s'] / 1e6, 1)
    res['GBs_t'] = round(row.nf * row.frame / res['ms_t'] / 1e6, 1)
    res['s_over_t'] = round(res['ms_s'] / res['ms_t'], 3)
    res['s_over_d'] = round(res['ms_s'] / res['ms_d'], 3)
    res['below_decode'] = bool(res['ms_s'] < res['ms_d'])
    res['within_aim'] = bool(res['s_over_t'] <= AIM)
    del out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--windows', type=int, default=3, help='1 GiB windows of random bytes taking turns')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_states.py measures on the GPU: none found")
    from baseband_amd import _lib, kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    kernels.init()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    nwin = max(2, args.windows)
    image = torch.randint(0, 256, (nwin * WINDOW,), dtype=torch.uint8, device=dev, generator=g)
    zeros = torch.zeros(2 * WINDOW, dtype=torch.uint8, device=dev)
    V, M = _lib.CODER_VDIF, _lib.CODER_MARK5B
    rows = [Row('vdif 8032 B, 2-bit, chunk 1, random', V, 2, 1, 8032, 32),
            Row('mark5b 10016 B, 2-bit, chunk 16, random', M, 2, 16, 10016, 16),
            Row('vdif 8032 B, 8-bit, chunk 2, random', V, 8, 2, 8032, 32),
            Row('vdif 8032 B, 2-bit, chunk 1, all zero', V, 2, 1, 8032, 32, zeros=True)]
    print("# device: {}; {} windows of 1 GiB taking turns; reps {} (median), 2 warm-up rounds".format(
        torch.cuda.get_device_name(dev), nwin, args.reps))
    print("# (s) bb_count_states  (t) bb_touch  (d) float32 bb_decode_frames")
    print("# {:<42s} {:>8s} {:>8s} {:>8s}  {:>8s} {:>8s}  {:>6s} {:>6s}  s<d  s<=1.3t".format(
        'row', 's ms', 't ms', 'd ms', 's GB/s', 't GB/s', 's/t', 's/d'))
    out = []
    for row in rows:
        r = run_row(row, zeros if row.zeros else image, args.reps)
        out.append(r)
        print("  {:<42s} {:8.4f} {:8.4f} {:8.4f}  {:8.1f} {:8.1f}  {:6.3f} {:6.3f}  {:<3s}  {}{}".format(
            r['row'], r['ms_s'], r['ms_t'], r['ms_d'], r['GBs_s'], r['GBs_t'], r['s_over_t'], r['s_over_d'],
            'yes' if r['below_decode'] else 'NO', 'yes' if r['within_aim'] else 'no',
            '' if r['codes_counted_ok'] else '  COUNT TOTAL WRONG'))
        sys.stdout.flush()
    for r in out:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
