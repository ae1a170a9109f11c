#!/usr/bin/env python
"""Time of ``fh.coherence_series()`` on GUPPI raw and DADA streams (bb_i8_coherence,
k_coherence.h) against the read-only ceiling, against ``fh.moment_series()`` of the same bytes
and against what a user did for the same answer before, on one GPU.  The method, the image
and the rows are those of tools/bench_moments.py.

A file image of 4 GiB (frames of 64 MiB of int8 payload) lies in HBM and a reader is opened on
it.  For every row -- a format, at a short bin of 256 samples and at one bin for the whole
request -- these are timed over one WINDOW of 16 frames, taking turns inside every repetition,
each on the NEXT window of the image so that no input is still in the 256 MiB memory-side
cache:
  (c) ``fh.coherence_series(bin, count)``: the new pass, as a user calls it,
  (k) its kernel launch alone (``kernels.i8_coherence`` on the same frames),
  (t) ``bb_touch`` of the same bytes: the library's read-once launch, the ceiling,
  (m) ``fh.moment_series(bin, count)`` of the same bytes, and (n) its kernel launch alone,
  (f) ``fh.coherence_series(bin, count, packed=False)``: read() in pieces plus the int64
      reduction by torch, the code every other stream falls back to.
GPU events around the calls on the launching stream; two warm-up rounds.  Reported: all
times of (c) and (f), the medians of the others, the window's bytes over the median of (k),
and the condition the design answers to: the SLOWEST (c) is faster than the FASTEST (f) in
every row (exit status 1 otherwise).  t(k) / t(t) and t(k) / t(n) are recorded, not judged.
Both answers of a row are compared: they must be equal.

    python tools/bench_coherence.py [--reps 5] [--windows 4] > profiles/coherence.log
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_moments import FRAMES, PAYLOAD, ROWS, header_of, timed    # noqa: E402


def run_row(name, kind, npol, nchan, image, windows, reps):
    from baseband_amd import _lib, kernels
    assert npol == 2
    hdr, opener, layout, spf = header_of(kind, npol, nchan)
    frame = hdr.size + PAYLOAD
    nframes = windows * FRAMES
    assert nframes * frame <= image.numel()
    img = image[:nframes * frame]
    dev_hdr = torch.from_numpy(hdr.copy()).cuda()
    for f in range(nframes):
        img[f * frame:f * frame + hdr.size] = dev_hdr
    count = FRAMES * spf
    nbytes = FRAMES * frame
    results = []
    with opener(img, 'rs') as fh:
        assert fh.shape[0] == nframes * spf and fh._header_nbytes == hdr.size and fh._frame_nbytes == frame
        for bin_samples in (256, count):
            nbins = -(-count // bin_samples)
            turn = [0]

            def window():
                turn[0] += 1
                return turn[0] % windows

            def new():
                fh.seek(window() * count)
                return fh.coherence_series(bin_samples, count)

            def kernel():
                w = img[window() * nbytes:][:nbytes]
                return kernels.i8_coherence(w, FRAMES, layout, nchan, spf, 0, spf, bin_samples, nbins,
                                            src0=hdr.size, src_stride=frame)

            def touch():
                w = img[window() * nbytes:][:nbytes]
                _lib.check(_lib.lib.bb_touch(ctypes.c_void_p(w.data_ptr()), nbytes, kernels._stream(w)), 'bb_touch')

            def moments():
                fh.seek(window() * count)
                return fh.moment_series(bin_samples, count)

            def moments_kernel():
                w = img[window() * nbytes:][:nbytes]
                return kernels.i8_moments(w, FRAMES, layout, npol, nchan, 2, spf, 0, spf, bin_samples, nbins,
                                          src0=hdr.size, src_stride=frame)

            def fallback():
                fh.seek(window() * count)
                return fh.coherence_series(bin_samples, count, packed=False)

            # the two answers agree (on one window), and the kernel is the one that gave the first
            fh.seek(0)
            a = fh.coherence_series(bin_samples, count, packed=True)
            assert _lib.last_kernel().startswith('k_i8_coherence'), _lib.last_kernel()
            note = _lib.last_kernel()
            assert torch.equal(a, fh.coherence_series(bin_samples, count, packed=False))
            del a
            legs = (('c', new), ('k', kernel), ('t', touch), ('m', moments), ('n', moments_kernel), ('f', fallback))
            times = {key: [] for key, _ in legs}
            for rep in range(reps + 2):
                for key, fn in legs:
                    ms, out = timed(fn)
                    del out
                    if rep >= 2:
                        times[key].append(ms)
            med = {k: float(np.median(v)) for k, v in times.items()}
            ok = max(times['c']) < min(times['f'])
            results.append(dict(row=name, bin_samples=bin_samples, nbins=nbins, window_bytes=nbytes, kernel=note,
                                coherence_series_ms=[round(x, 3) for x in times['c']],
                                fallback_ms=[round(x, 3) for x in times['f']],
                                kernel_ms=round(med['k'], 3), touch_ms=round(med['t'], 3),
                                moment_series_ms=round(med['m'], 3), moments_kernel_ms=round(med['n'], 3),
                                kernel_tb_s=round(nbytes / med['k'] / 1e9, 3), touch_tb_s=round(nbytes / med['t'] / 1e9, 3),
                                kernel_over_touch=round(med['k'] / med['t'], 2),
                                kernel_over_moments_kernel=round(med['k'] / med['n'], 2),
                                fallback_over_new=round(min(times['f']) / max(times['c']), 1), condition_holds=ok))
            r = results[-1]
            print("{:40s} bin {:>9d}  (c) {:7.3f} .. {:7.3f} ms  (k) {:6.3f} ms {:5.2f} TB/s  (t) {:6.3f} ms {:5.2f} TB/s  "
                  "(m) {:6.3f} ms  (n) {:6.3f} ms  (f) {:8.3f} .. {:8.3f} ms  slowest (c) vs fastest (f): x{:<6.1f} {}".format(
                      name, bin_samples, min(times['c']), max(times['c']), med['k'], r['kernel_tb_s'], med['t'], r['touch_tb_s'],
                      med['m'], med['n'], min(times['f']), max(times['f']), r['fallback_over_new'], 'holds' if ok else 'FAILS'),
                  flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--windows', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_coherence.py needs a GPU"
    torch.cuda.set_device(0)
    total = args.windows * FRAMES * (PAYLOAD + 16384)
    image = torch.empty(total, dtype=torch.uint8, device='cuda')
    for lo in range(0, total, 1 << 28):
        image[lo:lo + (1 << 28)].random_(0, 256)
    print("# tools/bench_coherence.py: {} windows of {} frames x {} MiB on {}; {} timed repetitions after 2 warm-up rounds".format(
        args.windows, FRAMES, PAYLOAD >> 20, torch.cuda.get_device_name(0), args.reps))
    print("# (c) fh.coherence_series  (k) its kernel launch alone  (t) bb_touch of the same bytes  (m) fh.moment_series  "
          "(n) its kernel launch alone  (f) coherence_series(packed=False)")
    results = []
    for name, kind, npol, nchan in ROWS:
        results += run_row(name, kind, npol, nchan, image, args.windows, args.reps)
    print(json.dumps(dict(bench='coherence', rows=results)))
    return 0 if all(r['condition_holds'] for r in results) else 1


if __name__ == '__main__':
    sys.exit(main())
