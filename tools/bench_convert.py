#!/usr/bin/env python
"""Kernel time of format conversion on the packed bytes (bb_repack_frames, k_repack.h)
against what the same conversion costs without it, on one GPU.

For every row three things are timed, taking turns inside every repetition, on the same
1 GiB of frames at a fixed stride, resident in HBM:
  (r)   bb_repack_frames: N packed bytes in, N out,
  (d+e) what `fw.write(fr.read(n))` launches for the same conversion: the float32
        bb_decode_frames, the writer's permutation to payload order where the output has
        more than one thread, and bb_encode_flat: 34 N of traffic at 2 bits, 10 N at 8,
  (c)   bb_copy_frames over the same payloads: the same algorithmic traffic with no bit
        work (for the record; no threshold).
HIP events around the launches on the launching stream; two warm-up rounds; every launch
takes the NEXT 1 GiB window of a larger image, so that no input is still in the 256 MiB
memory-side cache.  Reported: the median times, the bytes read over that time for (r),
and the relation the design answers to: (r) below (d+e) in every row.  Once per row the
bytes of (r) are compared with the bytes of (d+e) on the device: they must be equal.

    python tools/bench_convert.py [--reps 7] [--windows 3] > profiles/convert.log
"""
import argparse
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
    def __init__(self, name, shape, bps, coders, slots_in, slots_out, payload_in, hdr, payload_out):
        self.name, self.shape, self.bps, self.coders = name, shape, bps, coders
        (self.nslot_in, self.chunk_in), (self.nslot_out, self.chunk_out) = slots_in, slots_out
        self.payload_in, self.hdr, self.payload_out = payload_in, hdr, payload_out
        self.frame = hdr + payload_in                       # bytes of a frame-slot in the file
        set_nbytes = self.frame * self.nslot_in
        r_in = payload_in * 8 // bps // self.chunk_in
        self.r_out = payload_out * 8 // bps // self.chunk_out
        # whole output frames: as many input frame sets as give a whole number of them
        step = self.r_out // int(np.gcd(r_in, self.r_out))
        self.nf = WINDOW // set_nbytes // step * step
        self.nrows = self.nf * r_in
        self.nout = self.nrows // self.r_out
        self.nbytes = self.nf * self.nslot_in * payload_in   # packed bytes in = out


def run_row(row, image, reps):
    import baseband_amd
    from baseband_amd import kernels
    dev = image.device
    nwin = image.numel() // WINDOW
    ncomp = row.nslot_in * row.chunk_in
    packed = torch.empty(row.nbytes, dtype=torch.uint8, device=dev)
    plain = torch.empty(row.nbytes // 4, dtype=torch.float32, device=dev)
    floats = baseband_amd.empty_output(row.nrows * ncomp, torch.float32, dev)
    turn = [0]

    def window():
        k = turn[0] % nwin
        return image[k * WINDOW:(k + 1) * WINDOW]

    def r():
        return kernels.repack_frames(window(), row.nf, row.payload_in, row.bps, row.coders[0], row.chunk_in,
                                     row.nslot_in, row.coders[1], row.chunk_out, row.nslot_out, row.payload_out,
                                     src0=row.hdr, src_stride=row.frame, out=packed)

    def de():
        x = kernels.decode_frames(window(), row.nf, row.payload_in, row.coders[0], row.bps, chunk=row.chunk_in,
                                  nslot=row.nslot_in, src0=row.hdr, src_stride=row.frame, out=floats)
        if row.nslot_out > 1:                               # (set, sample, thread, chan) -> payload order
            x = x.view(row.nout, row.r_out, row.nslot_out, row.chunk_out).permute(0, 2, 1, 3).contiguous()
        return kernels.encode_flat(x.reshape(-1), row.coders[1], row.bps)

    def c():
        return kernels.copy_frames(window(), row.nf * row.nslot_in, row.payload_in, src0=row.hdr,
                                   src_stride=row.frame, out=plain)

    same = torch.equal(r(), de())                           # (the same window: `turn` has not moved)
    ts = {'r': [], 'de': [], 'c': []}
    for k in range(reps + 2):
        for key, fn in (('r', r), ('de', de), ('c', c)):
            turn[0] += 1
            ms = timed(fn)
            if k >= 2:
                ts[key].append(ms)
    res = {'row': row.name, 'shape': row.shape, 'bps': row.bps, 'frame_sets': row.nf, 'slots_in': row.nslot_in,
           'chunk_in': row.chunk_in, 'slots_out': row.nslot_out, 'chunk_out': row.chunk_out,
           'payload_in': row.payload_in, 'payload_out': row.payload_out, 'packed_GB': round(row.nbytes / 1e9, 4),
           'windows': nwin, 'same_bytes_as_decode_encode': bool(same)}
    for key in ts:
        res['ms_' + key] = round(float(np.median(ts[key])), 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
    res['GBs_r_read'] = round(row.nbytes / res['ms_r'] / 1e6, 1)
    res['r_over_c'] = round(res['ms_r'] / res['ms_c'], 3)
    res['de_over_r'] = round(res['ms_de'] / res['ms_r'], 2)
    res['below_decode_and_encode'] = bool(res['ms_r'] < res['ms_de'])
    del packed, plain, floats
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--windows', type=int, default=3, help='1 GiB windows of random bytes taking turns')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_convert.py measures on the GPU: none found")
    from baseband_amd import _lib, kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    kernels.init()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    nwin = max(2, args.windows)
    image = torch.randint(0, 256, (nwin * WINDOW,), dtype=torch.uint8, device=dev, generator=g)
    V, M = _lib.CODER_VDIF, _lib.CODER_MARK5B
    rows = [Row('mark5b 16 ch -> vdif 1 x 16, frames re-cut', 'a', 2, (M, V), (1, 16), (1, 16), 10000, 16, 8000),
            Row('vdif 8 x 1 -> vdif 1 x 8 (thread merge)', 'b', 2, (V, V), (8, 1), (1, 8), 8000, 32, 8000),
            Row('vdif 1 x 8 -> vdif 8 x 1 (thread split)', 'c', 2, (V, V), (1, 8), (8, 1), 8000, 32, 8000),
            Row('vdif 8-bit 1 x 2 -> frames re-cut', 'a', 8, (V, V), (1, 2), (1, 2), 8000, 32, 5000)]
    print("# device: {}; {} windows of 1 GiB taking turns; reps {} (median), 2 warm-up rounds".format(
        torch.cuda.get_device_name(dev), nwin, args.reps))
    print("# (r) bb_repack_frames  (d+e) float32 bb_decode_frames [+ permute] + bb_encode_flat  (c) bb_copy_frames")
    print("# {:<44s} {:>5s} {:>8s} {:>9s} {:>8s}  {:>10s} {:>6s} {:>8s}  same  r<d+e".format(
        'row', 'shape', 'r ms', 'd+e ms', 'c ms', 'r GB/s in', 'r/c', '(d+e)/r'))
    out = []
    for row in rows:
        res = run_row(row, image, args.reps)
        out.append(res)
        print("  {:<44s} {:>5s} {:8.4f} {:9.4f} {:8.4f}  {:10.1f} {:6.3f} {:8.2f}  {:<4s}  {}".format(
            res['row'], res['shape'], res['ms_r'], res['ms_de'], res['ms_c'], res['GBs_r_read'], res['r_over_c'],
            res['de_over_r'], 'yes' if res['same_bytes_as_decode_encode'] else 'NO',
            'yes' if res['below_decode_and_encode'] else 'NO'))
        sys.stdout.flush()
    for res in out:
        print(json.dumps(res))


if __name__ == '__main__':
    main()
