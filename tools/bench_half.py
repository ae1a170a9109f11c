#!/usr/bin/env python
"""Kernel time of the 16-bit decode (k_half.h) against the float32 decode and
against today's route to 16-bit samples, on one GPU.

For every row three things are timed, taking turns inside every repetition:
  (a) the float32 launch (the kernels every earlier release ships),
  (b) the launch with out_dtype=float16 (bfloat16 runs the same kernel on another table),
  (c) the float32 launch followed by the conversion pass of ``.to(torch.float16)``
      (into a destination made beforehand: the allocation is not timed).
HIP events around the launches on the launching stream; two warm-up rounds;
every launch decodes the NEXT window of a larger random image (no input is
still in the 256 MiB memory-side cache) into the next of a few output buffers
taking turns (outputs from baseband_amd.empty_output).  Reported: the median
time, and the algorithmic bytes (frame bytes read + samples written; for (c)
also the float32 samples read again and the 16-bit ones written) over that
time as a fraction of the 8 TB/s HBM peak.

    python tools/bench_half.py [--reps 7] [--max-log2 19] > profiles/half_output.log
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Row:
    """One geometry: `nf` frame(set)s of `nslot` frames of `frame` bytes (payload behind `hdr`)."""

    def __init__(self, name, coder, bps, frame, hdr, nf, nslot=1, chunk=1, cplx=False):
        self.name, self.coder, self.bps, self.frame, self.hdr, self.nf = name, coder, bps, frame, hdr, nf
        self.nslot, self.chunk, self.cplx = nslot, chunk, cplx
        self.pn = frame - hdr
        self.nelem = nf * nslot * self.pn * 8 // bps
        self.in_bytes = nf * nslot * frame

    def bytes_moved(self, which):
        out32, out16 = self.nelem * 4, self.nelem * 2
        return {'a': self.in_bytes + out32, 'b': self.in_bytes + out16,
                'c': self.in_bytes + out32 + out32 + out16}[which]


def run_row(row, image, reps, tiles=0):
    import baseband_amd
    from baseband_amd import kernels, _lib
    dev = image.device
    win_bytes = row.in_bytes
    nwin = max(1, image.numel() // win_bytes)
    free = torch.cuda.mem_get_info(dev)[0]
    nrot = int(max(1, min(3, (free - (24 << 30)) // max(1, row.nelem * 8))))
    o32 = [baseband_amd.empty_output(row.nelem, torch.float32, dev) for _ in range(nrot)]
    o16 = [kernels.empty_decoded(row.nelem, dev, torch.float16) for _ in range(nrot)]
    c16 = [kernels.empty_decoded(row.nelem, dev, torch.float16) for _ in range(nrot)]
    src = None
    if row.nslot > 1:
        src = (torch.arange(row.nf * row.nslot, dtype=torch.int64, device=dev) * row.frame + row.hdr)
    turn = [0]

    def launch(dtype, out):
        k = turn[0] % nwin
        win = image[k * win_bytes:(k + 1) * win_bytes]
        if src is None:
            kernels.decode_frames(win, row.nf, row.pn, row.coder, row.bps, src0=row.hdr, src_stride=row.frame,
                                  out=out, out_dtype=dtype)
        else:
            kernels.decode_frames(win, row.nf, row.pn, row.coder, row.bps, chunk=row.chunk, nslot=row.nslot,
                                  src=src, complex_data=row.cplx, out=out, out_dtype=dtype)

    def a():
        launch(torch.float32, o32[turn[0] % nrot])

    def b():
        if tiles:
            kernels.tune(_lib.TUNE_LUT_TILES, tiles)
        try:
            launch(torch.float16, o16[turn[0] % nrot])
        finally:
            if tiles:
                kernels.tune(_lib.TUNE_LUT_TILES, 0)

    def c():
        o = o32[turn[0] % nrot]
        launch(torch.float32, o)
        c16[turn[0] % nrot].copy_(o)

    ts = {'a': [], 'b': [], 'c': []}
    names = {}
    for r in range(reps + 2):
        for key, fn in (('a', a), ('b', b), ('c', c)):
            turn[0] += 1
            t = timed(fn)
            if key != 'c':
                names[key] = _lib.last_kernel()
            if r >= 2:
                ts[key].append(t)
    # the two routes to 16 bits agree bit for bit (same window, same turn)
    turn[0] += 1
    b()
    c()
    k = turn[0] % nrot
    agree = bool(torch.equal(o16[k].view(torch.int16), c16[k].view(torch.int16)))
    res = {'row': row.name, 'frames': row.nf, 'in_GB': round(row.in_bytes / 1e9, 3),
           'out32_GB': round(row.nelem * 4 / 1e9, 3), 'windows': nwin, 'outputs_taking_turns': nrot,
           'tiles_per_wave_knob': tiles, 'kernel_a': names['a'], 'kernel_b': names['b'], 'b_equals_c_bitwise': agree}
    for key in 'abc':
        ms = float(np.median(ts[key]))
        res['ms_' + key] = round(ms, 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
        res['frac_' + key] = round(row.bytes_moved(key) / ms / 1e6 / HBM_PEAK_GBS, 4)
    res['b_over_a_time'] = round(res['ms_b'] / res['ms_a'], 4)
    res['bytes_b_over_a'] = round(row.bytes_moved('b') / row.bytes_moved('a'), 4)
    res['ordered_b_lt_a_lt_c'] = bool(res['ms_b'] < res['ms_a'] < res['ms_c'])
    del o32, o16, c16
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--max-log2', type=int, default=19, help='largest 2-bit launch: at most 2^N frames')
    ap.add_argument('--image-gib', type=float, default=8.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_half.py measures on the GPU: none found")
    from baseband_amd import _lib, kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    kernels.init()
    free = torch.cuda.mem_get_info(dev)[0]
    # the largest 2-bit launch whose float32 AND 16-bit outputs fit (one of each for the
    # three routes: 128000 + 2 * 64000 bytes per frame) next to two windows of input
    lg = args.max_log2
    while lg > 15 and (1 << lg) * (128000 + 2 * 64000 + 2 * 8032) > free - (12 << 30):
        lg -= 1
    img_bytes = max(int(args.image_gib * (1 << 30)), 2 * (1 << lg) * 8032)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    image = torch.randint(0, 256, (img_bytes,), dtype=torch.uint8, device=dev, generator=g)
    V, M, I = _lib.CODER_VDIF, _lib.CODER_MARK5B, _lib.CODER_INT
    rows = [Row('vdif 2-bit 8032 B, 2^13', V, 2, 8032, 32, 1 << 13),
            Row('vdif 2-bit 8032 B, 2^15', V, 2, 8032, 32, 1 << 15),
            Row('vdif 2-bit 8032 B, 2^{} (largest that fits)'.format(lg), V, 2, 8032, 32, 1 << lg),
            Row('mark5b 2-bit 10016 B, 2^15', M, 2, 10016, 16, 1 << 15),
            Row('vdif 8-bit 8032 B, 2^17', V, 8, 8032, 32, 1 << 17),
            Row('int8 8192 B, 2^17', I, 8, 8192, 0, 1 << 17),
            Row('vdif 1-bit 8032 B, 2^14', V, 1, 8032, 32, 1 << 14),
            Row('vdif 4-bit 8032 B, 2^16', V, 4, 8032, 32, 1 << 16),
            # the geometry of smoke() (8 threads x 4 channels, 2-bit complex, 4000-byte payloads)
            # scaled to 1 GiB of input: the thread-interleave kernel against k_decode_gather / _rows_pipe
            Row('interleave 8 thr x chunk 8, 2-bit, 1 GiB in', V, 2, 4032, 32, (1 << 30) // (8 * 4032), nslot=8,
                chunk=8, cplx=True)]
    print("# device: {}; free {:.1f} GiB; image {:.1f} GiB; reps {} (median), 2 warm-up rounds".format(
        torch.cuda.get_device_name(dev), free / 2 ** 30, img_bytes / 2 ** 30, args.reps))
    print("# {:<46s} {:>9s} {:>9s} {:>9s}   {:>6s} {:>6s} {:>6s}  {:>6s} {:>6s}  ok".format(
        'row', 'a ms', 'b ms', 'c ms', 'a/pk', 'b/pk', 'c/pk', 'tb/ta', 'Bb/Ba'))
    out = []

    def show(r, tag=''):
        print("  {:<46s} {:9.4f} {:9.4f} {:9.4f}   {:6.4f} {:6.4f} {:6.4f}  {:6.4f} {:6.4f}  {}{}".format(
            r['row'] + tag, r['ms_a'], r['ms_b'], r['ms_c'], r['frac_a'], r['frac_b'], r['frac_c'],
            r['b_over_a_time'], r['bytes_b_over_a'], 'yes' if r['ordered_b_lt_a_lt_c'] else 'NO',
            '' if r['b_equals_c_bitwise'] else '  (b) != (c) BITWISE'))
        sys.stdout.flush()

    def attempt(row, **kw):
        try:
            r = run_row(row, image, args.reps, **kw)
        except torch.cuda.OutOfMemoryError as exc:          # (a row that does not fit is reported, the rest still run)
            torch.cuda.empty_cache()
            print("  {:<46s} not measured: {}".format(row.name, str(exc).splitlines()[0][:100]))
            return None
        out.append(r)
        return r

    for row in rows:
        r = attempt(row)
        if r:
            show(r)
    # the geometry knob of the contiguous kernel (tiles of 256 input bytes per wave and work item;
    # default 8, 4 for 1-bit): the 2-bit rows again with 2, 4 and 6
    for row in rows[1:3]:
        for tiles in (2, 4, 6):
            r = attempt(row, tiles=tiles)
            if r:
                show(r, ' [tiles {}]'.format(tiles))
    for r in out:
        print(json.dumps(r))


if __name__ == '__main__':
    main()
