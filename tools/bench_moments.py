#!/usr/bin/env python
"""Time of ``fh.moment_series()`` on GUPPI raw and DADA streams (bb_i8_moments, k_moments.h)
against the read-only ceiling and against what a user did for the same answer before, on
one GPU.

A file image of a few GiB (frames of 64 MiB of int8 payload) lies in HBM and a reader is
opened on it.  For every row -- a format, at a short bin of 256 samples and at one bin for
the whole request -- four things are timed over one WINDOW of frames, taking turns inside
every repetition, each on the NEXT window of the image so that no input is still in the
256 MiB memory-side cache:
  (m) ``fh.moment_series(bin, count)``: the new pass, as a user calls it,
  (k) its kernel launch alone (``kernels.i8_moments`` on the same frames),
  (t) ``bb_touch`` of the same bytes: the library's read-once launch, the ceiling,
  (f) ``fh.moment_series(bin, count, packed=False)``: read() in pieces plus the int64
      reduction by torch, the code every other stream falls back to.
GPU events around the calls on the launching stream; two warm-up rounds.  Reported: all
times of (m) and (f), the medians of (k) and (t), the window's bytes over the median of
(k), and the condition the design answers to: the SLOWEST (m) is faster than the FASTEST
(f) in every row (exit status 1 otherwise).  The distance to (t) is recorded, not judged.
Both answers of a row are compared: they must be equal.

    python tools/bench_moments.py [--reps 5] [--windows 4] > profiles/moments.log
"""
import argparse
import ctypes
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAYLOAD = 64 << 20              # bytes of a frame's payload
FRAMES = 16                     # frames of a window: 1 GiB


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def header_of(kind, npol, nchan, payload=PAYLOAD):
    """(header bytes, opener, layout, samples per frame) of a frame of `payload` bytes of complex int8."""
    from baseband_amd import _lib, dada, guppi
    spf = payload // (npol * nchan * 2)
    t0 = np.datetime64('2020-02-02T02:02:02')
    if kind.startswith('guppi'):
        cf = kind == 'guppi_cf'
        h = guppi.GUPPIHeader.fromvalues(time=t0, sample_rate=1e6, samples_per_frame=spf, overlap=0, npol=npol, nchan=nchan,
                                         pktsize=8192, bps=8, pktfmt='1SFA' if cf else 'SIMPLE')
        layout, opener = (_lib.MOMENTS_GUPPI_CF if cf else _lib.MOMENTS_GUPPI_TF), guppi.open
    else:
        h = dada.DADAHeader.fromvalues(time=t0, sample_rate=1e6, samples_per_frame=spf, npol=npol, nchan=nchan, bps=8,
                                       complex_data=True)
        layout, opener = _lib.MOMENTS_ROWS, dada.open
    assert h.payload_nbytes == payload, (h.payload_nbytes, payload)
    f = io.BytesIO()
    h.tofile(f)
    return np.frombuffer(f.getvalue(), np.uint8), opener, layout, spf


ROWS = [('GUPPI channels first, 64 chan x 2 pol', 'guppi_cf', 2, 64),
        ('GUPPI time first, 64 chan x 2 pol', 'guppi_tf', 2, 64),
        ('DADA 2 pol x 1 chan', 'dada', 2, 1),
        ('DADA 2 pol x 64 chan', 'dada', 2, 64)]


def run_row(name, kind, npol, nchan, image, windows, reps):
    from baseband_amd import _lib, kernels
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
                return fh.moment_series(bin_samples, count)

            def kernel():
                w = img[window() * nbytes:][:nbytes]
                return kernels.i8_moments(w, FRAMES, layout, npol, nchan, 2, spf, 0, spf, bin_samples, nbins,
                                          src0=hdr.size, src_stride=frame)

            def touch():
                w = img[window() * nbytes:][:nbytes]
                _lib.check(_lib.lib.bb_touch(ctypes.c_void_p(w.data_ptr()), nbytes, kernels._stream(w)), 'bb_touch')

            def fallback():
                fh.seek(window() * count)
                return fh.moment_series(bin_samples, count, packed=False)

            # the two answers agree (on one window), and the kernel is the one that gave the first
            fh.seek(0)
            a = fh.moment_series(bin_samples, count, packed=True)
            assert _lib.last_kernel().startswith('k_i8_moments'), _lib.last_kernel()
            note = _lib.last_kernel()
            assert torch.equal(a, fh.moment_series(bin_samples, count, packed=False))
            del a
            times = {'m': [], 'k': [], 't': [], 'f': []}
            for rep in range(reps + 2):
                for key, fn in (('m', new), ('k', kernel), ('t', touch), ('f', fallback)):
                    ms, out = timed(fn)
                    del out
                    if rep >= 2:
                        times[key].append(ms)
            med = {k: float(np.median(v)) for k, v in times.items()}
            ok = max(times['m']) < min(times['f'])
            results.append(dict(row=name, bin_samples=bin_samples, nbins=nbins, window_bytes=nbytes, kernel=note,
                                moment_series_ms=[round(x, 3) for x in times['m']],
                                fallback_ms=[round(x, 3) for x in times['f']],
                                kernel_ms=round(med['k'], 3), touch_ms=round(med['t'], 3),
                                kernel_tb_s=round(nbytes / med['k'] / 1e9, 3), touch_tb_s=round(nbytes / med['t'] / 1e9, 3),
                                kernel_over_touch=round(med['k'] / med['t'], 2),
                                fallback_over_new=round(min(times['f']) / max(times['m']), 1), condition_holds=ok))
            r = results[-1]
            print("{:40s} bin {:>9d}  (m) {:7.3f} .. {:7.3f} ms  (k) {:6.3f} ms {:5.2f} TB/s  (t) {:6.3f} ms {:5.2f} TB/s  "
                  "(f) {:8.3f} .. {:8.3f} ms  slowest (m) vs fastest (f): x{:<6.1f} {}".format(
                      name, bin_samples, min(times['m']), max(times['m']), med['k'], r['kernel_tb_s'], med['t'], r['touch_tb_s'],
                      min(times['f']), max(times['f']), r['fallback_over_new'], 'holds' if ok else 'FAILS'), flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--windows', type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_moments.py needs a GPU"
    torch.cuda.set_device(0)
    total = args.windows * FRAMES * (PAYLOAD + 16384)
    image = torch.empty(total, dtype=torch.uint8, device='cuda')
    for lo in range(0, total, 1 << 28):
        image[lo:lo + (1 << 28)].random_(0, 256)
    print("# tools/bench_moments.py: {} windows of {} frames x {} MiB on {}; {} timed repetitions after 2 warm-up rounds".format(
        args.windows, FRAMES, PAYLOAD >> 20, torch.cuda.get_device_name(0), args.reps))
    print("# (m) fh.moment_series  (k) its kernel launch alone  (t) bb_touch of the same bytes  (f) moment_series(packed=False)")
    results = []
    for name, kind, npol, nchan in ROWS:
        results += run_row(name, kind, npol, nchan, image, args.windows, args.reps)
    print(json.dumps(dict(bench='moments', rows=results)))
    return 0 if all(r['condition_holds'] for r in results) else 1


if __name__ == '__main__':
    sys.exit(main())
