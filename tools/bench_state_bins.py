#!/usr/bin/env python
"""Kernel time of the time-resolved sampler statistics (bb_count_states_bins,
k_state_bins.h) against what a user does for the same answer without it, on one GPU.

For every row five launches are timed, taking turns inside every repetition, on the
same 1 GiB of frames at a fixed stride:
  (b)   bb_count_states_bins: every payload byte read once, chunk << bps counters per
        bin added,
  (s)   bb_count_states on the same frames: the same pass without the time axis,
  (t)   bb_touch of the window: the library's read-once launch,
  (d)   the float32 bb_decode_frames launch of the same frames,
  (d+r) that decode plus the torch reduction a user writes today for a power series:
        ``x.square().view(nbins, n, ...).sum(1)``.
HIP events around the launches on the launching stream; two warm-up rounds; every
launch takes the NEXT 1 GiB window of a larger image, so that no input is still in the
256 MiB memory-side cache.  Reported: the median times, the window's bytes over that
time for (b), and the relation the design answers to: (b) below (d+r) in every row
whose counts are smaller than the bytes counted ("judged"; where a bin's counters are as
large as its bytes the row is recorded only).  Every launch's codes are counted on the
device: each exactly once.

    python tools/bench_state_bins.py [--reps 7] [--windows 3] > profiles/state_bins.log
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Row:
    def __init__(self, name, coder, bps, chunk, frame, hdr, bin_samples, zeros=False):
        self.name, self.coder, self.bps, self.chunk, self.frame, self.hdr = name, coder, bps, chunk, frame, hdr
        self.bin_samples, self.zeros = bin_samples, zeros
        self.pn = frame - hdr
        self.nf = WINDOW // frame
        self.nelem = self.nf * self.pn * 8 // bps
        self.nrows = self.nelem // chunk
        self.nbins = -(-self.nrows // bin_samples)


def run_row(row, image, reps):
    import baseband_amd
    from baseband_amd import kernels, _lib
    dev = image.device
    nwin = image.numel() // WINDOW
    out = baseband_amd.empty_output(row.nelem, torch.float32, dev)
    counts = torch.zeros((1, row.chunk, 1 << row.bps), dtype=torch.int64, device=dev)
    series = torch.zeros((1, row.nbins, row.chunk, 1 << row.bps), dtype=torch.int32, device=dev)
    whole_bins = row.nrows // row.bin_samples
    turn = [0]
    seen = [0, 0]                                           # codes every (b) launch added, and how many were right

    def window():
        k = turn[0] % nwin
        return image[k * WINDOW:(k + 1) * WINDOW]

    def b():
        kernels.count_states_bins(window(), row.nf, row.pn, row.bps, row.chunk, 1, row.bin_samples, row.nbins,
                                  src0=row.hdr, src_stride=row.frame, counts=series)

    def s():
        kernels.count_states(window(), row.nf, row.pn, row.bps, row.chunk, src0=row.hdr, src_stride=row.frame,
                             counts=counts)

    def t():
        w = window()
        _lib.check(_lib.lib.bb_touch(ctypes.c_void_p(w.data_ptr()), row.nf * row.frame, kernels._stream(w)), 'bb_touch')

    def d():
        return kernels.decode_frames(window(), row.nf, row.pn, row.coder, row.bps, chunk=row.chunk, src0=row.hdr,
                                     src_stride=row.frame, out=out)

    def dr():
        x = d()[:whole_bins * row.bin_samples * row.chunk]
        return x.square().view(whole_bins, row.bin_samples, row.chunk).sum(1)

    ts = {'b': [], 's': [], 't': [], 'd': [], 'dr': []}
    for r in range(reps + 2):
        for key, fn in (('b', b), ('s', s), ('t', t), ('d', d), ('dr', dr)):
            turn[0] += 1
            ms = timed(fn)
            if r >= 2:
                ts[key].append(ms)
            if key == 'b':
                # every code of this launch once: each bin's counters sum to its codes
                per_bin = series.sum((0, 2, 3), dtype=torch.int64)
                full = bool((per_bin[:whole_bins] == (seen[0] + 1) * row.bin_samples * row.chunk).all())
                seen[0] += 1
                seen[1] += int(full and int(per_bin.sum()) == seen[0] * row.nelem)
    decode_kernel = _lib.last_kernel()
    launches = reps + 2
    counts_nbytes = series.numel() * 4
    res = {'row': row.name, 'frames': row.nf, 'frame_nbytes': row.frame, 'bps': row.bps, 'chunk': row.chunk,
           'bin_samples': row.bin_samples, 'nbins': row.nbins, 'counts_MB': round(counts_nbytes / 1e6, 3),
           'window_GB': round(row.nf * row.frame / 1e9, 4), 'windows': nwin, 'decode_kernel': decode_kernel,
           'judged': bool(counts_nbytes < row.nf * row.pn),
           'codes_counted_ok': seen[1] == launches and int(counts.sum()) == launches * row.nelem}
    for key in ts:
        ms = float(np.median(ts[key]))
        res['ms_' + key] = round(ms, 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
    res['GBs_b'] = round(row.nf * row.frame / res['ms_b'] / 1e6, 1)
    res['b_over_s'] = round(res['ms_b'] / res['ms_s'], 3)
    res['b_over_dr'] = round(res['ms_b'] / res['ms_dr'], 3)
    res['below_decode_and_reduce'] = bool(res['ms_b'] < res['ms_dr'])
    del out, series
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--windows', type=int, default=3, help='1 GiB windows of random bytes taking turns')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_state_bins.py measures on the GPU: none found")
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
    rows = [Row('vdif 8032 B, 2-bit, chunk 1, bins of 256', V, 2, 1, 8032, 32, 256),
            Row('vdif 8032 B, 2-bit, chunk 1, bins of 1000', V, 2, 1, 8032, 32, 1000),
            Row('vdif 8032 B, 2-bit, chunk 1, bins of 32768', V, 2, 1, 8032, 32, 32768),
            Row('vdif 8032 B, 2-bit, chunk 1, bins of 2^22', V, 2, 1, 8032, 32, 1 << 22),
            Row('mark5b 10016 B, 2-bit, chunk 16, bins of 1000', M, 2, 16, 10016, 16, 1000),
            Row('vdif 8032 B, 8-bit, chunk 2, bins of 1000', V, 8, 2, 8032, 32, 1000),
            Row('vdif 8032 B, 8-bit, chunk 2, bins of 2^20', V, 8, 2, 8032, 32, 1 << 20),
            Row('vdif 8032 B, 2-bit, chunk 1, 1000, all zero', V, 2, 1, 8032, 32, 1000, zeros=True)]
    print("# device: {}; {} windows of 1 GiB taking turns; reps {} (median), 2 warm-up rounds".format(
        torch.cuda.get_device_name(dev), nwin, args.reps))
    print("# (b) bb_count_states_bins  (s) bb_count_states  (t) bb_touch  (d) float32 bb_decode_frames  "
          "(d+r) decode, square, sum per bin")
    print("# {:<46s} {:>8s} {:>8s} {:>8s} {:>8s} {:>9s}  {:>8s} {:>9s}  {:>6s} {:>7s}  judged  b<d+r".format(
        'row', 'b ms', 's ms', 't ms', 'd ms', 'd+r ms', 'b GB/s', 'counts MB', 'b/s', 'b/(d+r)'))
    out = []
    for row in rows:
        r = run_row(row, zeros if row.zeros else image, args.reps)
        out.append(r)
        print("  {:<46s} {:8.4f} {:8.4f} {:8.4f} {:8.4f} {:9.4f}  {:8.1f} {:9.3f}  {:6.3f} {:7.3f}  {:<6s}  {}{}".format(
            r['row'], r['ms_b'], r['ms_s'], r['ms_t'], r['ms_d'], r['ms_dr'], r['GBs_b'], r['counts_MB'],
            r['b_over_s'], r['b_over_dr'], 'yes' if r['judged'] else 'no',
            'yes' if r['below_decode_and_reduce'] else 'NO', '' if r['codes_counted_ok'] else '  COUNT TOTAL WRONG'))
        sys.stdout.flush()
    for r in out:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
