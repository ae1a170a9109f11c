#!/usr/bin/env python
"""Kernel time of conversion between sample widths on the packed bytes (bb_requant_frames,
k_requant.h) against what the same conversion costs without it, on one GPU.

For every row three things are timed, taking turns inside every repetition, on the same
1 GiB of frames at a fixed stride, resident in HBM:
  (q)   bb_requant_frames: N packed bytes in, N * bps_out / bps_in out,
  (d+e) what `convert`'s loop launches for the same conversion: the float32
        bb_decode_frames, the multiplication by the scale where there is one, the writer's
        permutation to payload order where the output has more than one thread, and
        bb_encode_flat at the output's width,
  (c)   bb_copy_frames over the input payloads: N in, N out with no bit work (for the
        record; no threshold).
HIP events around the launches on the launching stream; two warm-up rounds; every launch
takes the NEXT 1 GiB window of a larger image, so that no input is still in the 256 MiB
memory-side cache.  Reported: the median times, the bytes read over that time for (q),
and the relation the design answers to: (q) below (d+e) in every row.  Once per row the
bytes of (q) are compared with the bytes of (d+e) on the device: they must be equal.

    python tools/bench_requant.py [--reps 7] [--windows 3] > profiles/requant.log
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
    def __init__(self, name, coders, widths, slots, payload_in, hdr, payload_out, scale=None):
        self.name, self.coders, (self.bps_in, self.bps_out), self.scale = name, coders, widths, scale
        self.nslot, self.chunk = slots
        self.payload_in, self.hdr, self.payload_out = payload_in, hdr, payload_out
        self.frame = hdr + payload_in                       # bytes of a frame-slot in the file
        set_nbytes = self.frame * self.nslot
        r_in = payload_in * 8 // self.bps_in // self.chunk
        self.r_out = payload_out * 8 // self.bps_out // self.chunk
        # whole output frames: as many input frame sets as give a whole number of them
        step = self.r_out // int(np.gcd(r_in, self.r_out))
        self.nf = WINDOW // set_nbytes // step * step
        self.nrows = self.nf * r_in
        self.nout = self.nrows // self.r_out
        self.nbytes_in = self.nf * self.nslot * payload_in
        self.nbytes_out = self.nout * self.nslot * payload_out


def run_row(row, image, reps):
    import baseband_amd
    from baseband_amd import kernels
    dev = image.device
    nwin = image.numel() // WINDOW
    ncomp = row.nslot * row.chunk
    table = kernels.requant_table(row.coders[0], row.bps_in, row.coders[1], row.bps_out, row.scale)
    packed = torch.empty(row.nbytes_out, dtype=torch.uint8, device=dev)
    plain = torch.empty(row.nbytes_in // 4, dtype=torch.float32, device=dev)
    floats = baseband_amd.empty_output(row.nrows * ncomp, torch.float32, dev)
    gain = None if row.scale is None else float(np.float32(row.scale))
    turn = [0]

    def window():
        k = turn[0] % nwin
        return image[k * WINDOW:(k + 1) * WINDOW]

    def q():
        return kernels.requant_frames(window(), row.nf, row.payload_in, row.bps_in, row.chunk, row.nslot, row.bps_out,
                                      row.payload_out, table, src0=row.hdr, src_stride=row.frame, out=packed)

    def de():
        x = kernels.decode_frames(window(), row.nf, row.payload_in, row.coders[0], row.bps_in, chunk=row.chunk,
                                  nslot=row.nslot, src0=row.hdr, src_stride=row.frame, out=floats)
        if gain is not None:
            x.mul_(gain)
        if row.nslot > 1:                                   # (set, sample, thread, chan) -> payload order
            x = x.view(row.nout, row.r_out, row.nslot, row.chunk).permute(0, 2, 1, 3).contiguous()
        return kernels.encode_flat(x.reshape(-1), row.coders[1], row.bps_out)

    def c():
        return kernels.copy_frames(window(), row.nf * row.nslot, row.payload_in, src0=row.hdr,
                                   src_stride=row.frame, out=plain)

    same = torch.equal(q(), de())                           # (the same window: `turn` has not moved)
    ts = {'q': [], 'de': [], 'c': []}
    for k in range(reps + 2):
        for key, fn in (('q', q), ('de', de), ('c', c)):
            turn[0] += 1
            ms = timed(fn)
            if k >= 2:
                ts[key].append(ms)
    res = {'row': row.name, 'bps_in': row.bps_in, 'bps_out': row.bps_out, 'scale': row.scale, 'frame_sets': row.nf,
           'slots': row.nslot, 'chunk': row.chunk, 'payload_in': row.payload_in, 'payload_out': row.payload_out,
           'packed_in_GB': round(row.nbytes_in / 1e9, 4), 'packed_out_GB': round(row.nbytes_out / 1e9, 4),
           'windows': nwin, 'same_bytes_as_decode_encode': bool(same)}
    for key in ts:
        res['ms_' + key] = round(float(np.median(ts[key])), 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
    res['GBs_q_read'] = round(row.nbytes_in / res['ms_q'] / 1e6, 1)
    res['GBs_q_moved'] = round((row.nbytes_in + row.nbytes_out) / res['ms_q'] / 1e6, 1)
    res['q_over_c'] = round(res['ms_q'] / res['ms_c'], 3)
    res['de_over_q'] = round(res['ms_de'] / res['ms_q'], 2)
    res['below_decode_and_encode'] = bool(res['ms_q'] < res['ms_de'])
    del packed, plain, floats
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--windows', type=int, default=3, help='1 GiB windows of random bytes taking turns')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_requant.py measures on the GPU: none found")
    from baseband_amd import _lib, kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    kernels.init()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    nwin = max(2, args.windows)
    image = torch.randint(0, 256, (nwin * WINDOW,), dtype=torch.uint8, device=dev, generator=g)
    V, M = _lib.CODER_VDIF, _lib.CODER_MARK5B
    rows = [Row('vdif 8 -> 2 bits, 1 thread x 1', (V, V), (8, 2), (1, 1), 8000, 32, 8000),
            Row('vdif 2 -> 8 bits, 8 threads x 1', (V, V), (2, 8), (8, 1), 8000, 32, 8000),
            Row('mark5b 16 ch 2 bits -> vdif 4 bits', (M, V), (2, 4), (1, 16), 10000, 16, 8000),
            Row('vdif 2 -> 2 bits, 1 thread x 8, scale 0.5', (V, V), (2, 2), (1, 8), 8000, 32, 8000, 0.5)]
    print("# device: {}; {} windows of 1 GiB taking turns; reps {} (median), 2 warm-up rounds".format(
        torch.cuda.get_device_name(dev), nwin, args.reps))
    print("# (q) bb_requant_frames  (d+e) float32 bb_decode_frames [* scale] [+ permute] + bb_encode_flat  "
          "(c) bb_copy_frames")
    print("# {:<44s} {:>8s} {:>9s} {:>8s}  {:>10s} {:>11s} {:>6s} {:>8s}  same  q<d+e".format(
        'row', 'q ms', 'd+e ms', 'c ms', 'q GB/s in', 'q GB/s i+o', 'q/c', '(d+e)/q'))
    out = []
    for row in rows:
        res = run_row(row, image, args.reps)
        out.append(res)
        print("  {:<44s} {:8.4f} {:9.4f} {:8.4f}  {:10.1f} {:11.1f} {:6.3f} {:8.2f}  {:<4s}  {}".format(
            res['row'], res['ms_q'], res['ms_de'], res['ms_c'], res['GBs_q_read'], res['GBs_q_moved'], res['q_over_c'],
            res['de_over_q'], 'yes' if res['same_bytes_as_decode_encode'] else 'NO',
            'yes' if res['below_decode_and_encode'] else 'NO'))
        sys.stdout.flush()
    for res in out:
        print(json.dumps(res))
    return 0 if all(r['same_bytes_as_decode_encode'] and r['below_decode_and_encode'] for r in out) else 1


if __name__ == '__main__':
    sys.exit(main())
