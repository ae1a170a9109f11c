#!/usr/bin/env python
"""Kernel time of conversion between sample widths across thread layouts on the packed bytes
(bb_recode_frames, k_recode.h) against what the same conversion costs without it, on one GPU.

For every row three things are timed, taking turns inside every repetition, on the same
frames at a fixed stride, resident in HBM (1 GiB on the wider side of the conversion):
  (r)   bb_recode_frames: N packed bytes in, N * bps_out / bps_in out,
  (a)   the two kernels it fuses: bb_requant_frames into a temporary of the input's thread
        structure, then bb_repack_frames of the temporary into the output's,
  (b)   what the loop launches: the float32 bb_decode_frames, the multiplication by the scale,
        the writer's permutation to payload order where the output has more than one thread,
        and bb_encode_flat at the output's width.
HIP events around the launches on the launching stream; two warm-up rounds; every launch
takes the NEXT window of a larger image, so that no input is still in the 256 MiB
memory-side cache.  Reported: the median times and their spread (min .. max), the bytes moved
over the time of (r) and their share of the HBM peak, and the relation the design answers
to on its first row: (r) below (a) beyond the spread of (a), that is, the slowest (r) faster
than the fastest (a).  Once per row the bytes of (r) are compared with the bytes of (a) and
of (b) on the device: they must be equal.

    python tools/bench_recode.py [--reps 7] [--windows 3] > profiles/recode.log
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDE = 1 << 30                  # bytes of a window on the wider side
HBM_PEAK = 8.0e12               # bytes / s (MI355X, HBM3E)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Row:
    def __init__(self, name, widths, slots_in, slots_out, scale=0.9, payload_in=8000, hdr=32, payload_out=8000):
        self.name, (self.bps_in, self.bps_out), self.scale = name, widths, scale
        (self.nslot_in, self.chunk_in), (self.nslot_out, self.chunk_out) = slots_in, slots_out
        self.payload_in, self.hdr, self.payload_out = payload_in, hdr, payload_out
        self.frame = hdr + payload_in                       # bytes of a frame-slot in the file
        self.payload_tmp = payload_in * self.bps_out // self.bps_in     # (a): the input's structure at the output's width
        self.window = WIDE if self.bps_in >= self.bps_out else WIDE * self.bps_in // self.bps_out
        set_nbytes = self.frame * self.nslot_in
        r_in = payload_in * 8 // self.bps_in // self.chunk_in
        self.r_out = payload_out * 8 // self.bps_out // self.chunk_out
        # whole output frames: as many input frame sets as give a whole number of them
        step = self.r_out // int(np.gcd(r_in, self.r_out))
        self.nf = self.window // set_nbytes // step * step
        self.nrows = self.nf * r_in
        self.nout = self.nrows // self.r_out
        self.nbytes_in = self.nf * self.nslot_in * payload_in
        self.nbytes_out = self.nout * self.nslot_out * payload_out


def run_row(row, image, reps):
    import baseband_amd
    from baseband_amd import _lib, kernels
    dev = image.device
    V = _lib.CODER_VDIF
    nwin = image.numel() // row.window
    ncomp = row.nslot_in * row.chunk_in
    table = kernels.requant_table(V, row.bps_in, V, row.bps_out, row.scale)
    outs = {k: torch.empty(row.nbytes_out, dtype=torch.uint8, device=dev) for k in 'ra'}
    tmp = torch.empty(row.nf * row.nslot_in * row.payload_tmp, dtype=torch.uint8, device=dev)
    floats = baseband_amd.empty_output(row.nrows * ncomp, torch.float32, dev)
    gain = float(np.float32(row.scale))
    turn = [0]

    def window():
        k = turn[0] % nwin
        return image[k * row.window:(k + 1) * row.window]

    def r():
        return kernels.recode_frames(window(), row.nf, row.payload_in, row.bps_in, row.chunk_in, row.nslot_in,
                                     row.bps_out, row.chunk_out, row.nslot_out, row.payload_out, table,
                                     src0=row.hdr, src_stride=row.frame, out=outs['r'])

    def a():
        kernels.requant_frames(window(), row.nf, row.payload_in, row.bps_in, row.chunk_in, row.nslot_in, row.bps_out,
                               row.payload_tmp, table, src0=row.hdr, src_stride=row.frame, out=tmp)
        return kernels.repack_frames(tmp, row.nf, row.payload_tmp, row.bps_out, V, row.chunk_in, row.nslot_in, V,
                                     row.chunk_out, row.nslot_out, row.payload_out, src0=0, src_stride=row.payload_tmp,
                                     out=outs['a'])

    def b():
        x = kernels.decode_frames(window(), row.nf, row.payload_in, V, row.bps_in, chunk=row.chunk_in,
                                  nslot=row.nslot_in, src0=row.hdr, src_stride=row.frame, out=floats)
        x.mul_(gain)
        if row.nslot_out > 1:                               # (sample, component) -> payload order
            x = x.view(row.nout, row.r_out, row.nslot_out, row.chunk_out).permute(0, 2, 1, 3).contiguous()
        return kernels.encode_flat(x.reshape(-1), V, row.bps_out)

    got = r()                                               # (the same window: `turn` has not moved)
    same_a, same_b = torch.equal(got, a()), torch.equal(got, b())
    assert same_a, "bb_recode_frames and requantize + repack give different bytes: " + row.name
    ts = {'r': [], 'a': [], 'b': []}
    for k in range(reps + 2):
        for key, fn in (('r', r), ('a', a), ('b', b)):
            turn[0] += 1
            ms = timed(fn)
            if k >= 2:
                ts[key].append(ms)
    res = {'row': row.name, 'bps_in': row.bps_in, 'bps_out': row.bps_out, 'scale': row.scale, 'frame_sets': row.nf,
           'slots_in': [row.nslot_in, row.chunk_in], 'slots_out': [row.nslot_out, row.chunk_out],
           'payload_in': row.payload_in, 'payload_out': row.payload_out,
           'packed_in_GB': round(row.nbytes_in / 1e9, 4), 'packed_out_GB': round(row.nbytes_out / 1e9, 4),
           'windows': nwin, 'same_bytes_as_requant_repack': bool(same_a), 'same_bytes_as_decode_encode': bool(same_b)}
    for key in ts:
        res['ms_' + key] = round(float(np.median(ts[key])), 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
    res['GBs_r_read'] = round(row.nbytes_in / res['ms_r'] / 1e6, 1)
    res['GBs_r_moved'] = round((row.nbytes_in + row.nbytes_out) / res['ms_r'] / 1e6, 1)
    res['r_share_of_hbm_peak'] = round((row.nbytes_in + row.nbytes_out) / (res['ms_r'] * 1e-3) / HBM_PEAK, 3)
    res['a_over_r'] = round(res['ms_a'] / res['ms_r'], 3)
    res['b_over_r'] = round(res['ms_b'] / res['ms_r'], 2)
    res['a_spread'] = round((max(ts['a']) - min(ts['a'])) / res['ms_a'], 3)
    res['below_requant_repack_beyond_its_spread'] = bool(max(ts['r']) < min(ts['a']))
    del outs, tmp, floats
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--windows', type=int, default=3, help='1 GiB windows of random bytes taking turns')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_recode.py measures on the GPU: none found")
    from baseband_amd import kernels
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    kernels.init()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    nwin = max(2, args.windows)
    image = torch.randint(0, 256, (nwin * WIDE,), dtype=torch.uint8, device=dev, generator=g)
    rows = [Row('8 bits 8 threads x 1 -> 2 bits 1 x 8', (8, 2), (8, 1), (1, 8)),          # the headline row
            Row('4 bits 8 threads x 1 -> 2 bits 1 x 8', (4, 2), (8, 1), (1, 8)),
            Row('2 bits 1 x 8 -> 8 bits 8 threads x 1', (2, 8), (1, 8), (8, 1), 0.5),
            Row('8 bits 16 threads x 1 -> 2 bits 1 x 16', (8, 2), (16, 1), (1, 16))]
    print("# device: {}; {} windows taking turns, 1 GiB on the wider side; reps {} (median), 2 warm-up rounds".format(
        torch.cuda.get_device_name(dev), nwin, args.reps))
    print("# (r) bb_recode_frames  (a) bb_requant_frames into a temporary + bb_repack_frames  "
          "(b) float32 bb_decode_frames * scale [+ permute] + bb_encode_flat")
    print("# {:<40s} {:>8s} {:>17s} {:>8s} {:>17s} {:>8s}  {:>10s} {:>6s} {:>6s} {:>6s}  same  r<a".format(
        'row', 'r ms', 'min .. max', 'a ms', 'min .. max', 'b ms', 'r GB/s i+o', 'peak', 'a/r', 'b/r'))
    out = []
    for row in rows:
        res = run_row(row, image, args.reps)
        out.append(res)
        print("  {:<40s} {:8.4f} {:>17s} {:8.4f} {:>17s} {:8.4f}  {:10.1f} {:6.3f} {:6.3f} {:6.2f}  {:<4s}  {}".format(
            res['row'], res['ms_r'], '{:.4f} .. {:.4f}'.format(*res['ms_r_min_max']), res['ms_a'],
            '{:.4f} .. {:.4f}'.format(*res['ms_a_min_max']), res['ms_b'], res['GBs_r_moved'], res['r_share_of_hbm_peak'],
            res['a_over_r'], res['b_over_r'],
            'yes' if res['same_bytes_as_requant_repack'] and res['same_bytes_as_decode_encode'] else 'NO',
            'yes' if res['below_requant_repack_beyond_its_spread'] else 'NO'))
        sys.stdout.flush()
    for res in out:
        print(json.dumps(res))
    ok = all(r['same_bytes_as_requant_repack'] and r['same_bytes_as_decode_encode'] for r in out)
    return 0 if ok and out[0]['below_requant_repack_beyond_its_spread'] else 1


if __name__ == '__main__':
    sys.exit(main())
