#!/usr/bin/env python
"""Kernel time of requantizing with one gain per component on the packed bytes
(bb_recode_frames_tables, k_recode_tables.h) against the one-table kernel and against what the
same conversion costs without either, on one GPU.

For every row of tools/bench_recode.py three things are timed, taking turns inside every
repetition, on the same frames at a fixed stride, resident in HBM (1 GiB on the wider side of
the conversion, 8000-byte payloads):
  (t)   bb_recode_frames_tables with a table per component (tables resident on the device),
  (r)   bb_recode_frames with one table: t(t) / t(r) is the price of per-component tables,
  (b)   what the loop launches: the float32 bb_decode_frames, the broadcast product with the
        gains, the writer's permutation to payload order where the output has more than one
        thread, and bb_encode_flat at the output's width.
HIP events around the launches on the launching stream; two warm-up rounds; every launch takes
the NEXT window of a larger image, so that no input is still in the 256 MiB memory-side cache.
Reported: the median times and their spread (min .. max), t/r beside the spread of (r)'s own
runs, and the relation the design answers to on its first row: the slowest (t) faster than
the fastest (b).  Once per row the bytes of (t) are compared with the bytes of (b) on the
device: they must be equal.

    python tools/bench_recode_tables.py [--reps 7] [--windows 3] > profiles/recode_tables.log
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_recode import HBM_PEAK, WIDE, Row, timed     # noqa: E402  (the rows and the timing of the one-table bench)


def gains_of(row):
    """A gain per component at which the components' tables differ: a ladder of 8 steps, repeated."""
    k = np.arange(row.nslot_in * row.chunk_in, dtype=np.float32) % 8
    base, step = (0.5, 1.6) if row.bps_in < row.bps_out else (0.8, 1.25)
    return np.float32(base) * np.float32(step) ** k


def run_row(row, image, reps):
    import baseband_amd
    from baseband_amd import _lib, kernels
    dev = image.device
    V = _lib.CODER_VDIF
    nwin = image.numel() // row.window
    ncomp = row.nslot_in * row.chunk_in
    gains = gains_of(row)
    tables = kernels.requant_tables(V, row.bps_in, V, row.bps_out, gains)
    dtables = torch.from_numpy(tables).to(dev)
    dgains = torch.from_numpy(gains).to(dev)
    table = kernels.requant_table(V, row.bps_in, V, row.bps_out, row.scale)
    outs = {k: torch.empty(row.nbytes_out, dtype=torch.uint8, device=dev) for k in 'tr'}
    floats = baseband_amd.empty_output(row.nrows * ncomp, torch.float32, dev)
    turn = [0]

    def window():
        k = turn[0] % nwin
        return image[k * row.window:(k + 1) * row.window]

    def t():
        return kernels.recode_frames_tables(window(), row.nf, row.payload_in, row.bps_in, row.chunk_in, row.nslot_in,
                                            row.bps_out, row.chunk_out, row.nslot_out, row.payload_out, dtables,
                                            src0=row.hdr, src_stride=row.frame, out=outs['t'])

    def r():
        return kernels.recode_frames(window(), row.nf, row.payload_in, row.bps_in, row.chunk_in, row.nslot_in,
                                     row.bps_out, row.chunk_out, row.nslot_out, row.payload_out, table,
                                     src0=row.hdr, src_stride=row.frame, out=outs['r'])

    def b():
        x = kernels.decode_frames(window(), row.nf, row.payload_in, V, row.bps_in, chunk=row.chunk_in,
                                  nslot=row.nslot_in, src0=row.hdr, src_stride=row.frame, out=floats)
        x = x.view(row.nrows, ncomp).mul_(dgains)
        if row.nslot_out > 1:                               # (sample, component) -> payload order
            x = x.view(row.nout, row.r_out, row.nslot_out, row.chunk_out).permute(0, 2, 1, 3).contiguous()
        return kernels.encode_flat(x.reshape(-1), V, row.bps_out)

    same_b = torch.equal(t(), b())                          # (the same window: `turn` has not moved)
    ts = {'t': [], 'r': [], 'b': []}
    for k in range(reps + 2):
        for key, fn in (('t', t), ('r', r), ('b', b)):
            turn[0] += 1
            ms = timed(fn)
            if k >= 2:
                ts[key].append(ms)
    res = {'row': row.name, 'bps_in': row.bps_in, 'bps_out': row.bps_out, 'frame_sets': row.nf,
           'slots_in': [row.nslot_in, row.chunk_in], 'slots_out': [row.nslot_out, row.chunk_out],
           'payload_in': row.payload_in, 'payload_out': row.payload_out, 'distinct_tables': len({x.tobytes() for x in tables}),
           'packed_in_GB': round(row.nbytes_in / 1e9, 4), 'packed_out_GB': round(row.nbytes_out / 1e9, 4),
           'windows': nwin, 'same_bytes_as_decode_encode': bool(same_b)}
    for key in ts:
        res['ms_' + key] = round(float(np.median(ts[key])), 4)
        res['ms_' + key + '_min_max'] = [round(min(ts[key]), 4), round(max(ts[key]), 4)]
    res['GBs_t_moved'] = round((row.nbytes_in + row.nbytes_out) / res['ms_t'] / 1e6, 1)
    res['t_share_of_hbm_peak'] = round((row.nbytes_in + row.nbytes_out) / (res['ms_t'] * 1e-3) / HBM_PEAK, 3)
    res['t_over_r'] = round(res['ms_t'] / res['ms_r'], 3)
    res['r_spread'] = round((max(ts['r']) - min(ts['r'])) / res['ms_r'], 3)
    res['b_over_t'] = round(res['ms_b'] / res['ms_t'], 2)
    res['below_the_loop_beyond_its_spread'] = bool(max(ts['t']) < min(ts['b']))
    del outs, floats
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--windows', type=int, default=3, help='1 GiB windows of random bytes taking turns')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_recode_tables.py measures on the GPU: none found")
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
    print("# (t) bb_recode_frames_tables, a table per component  (r) bb_recode_frames, one table  "
          "(b) float32 bb_decode_frames * gains [+ permute] + bb_encode_flat")
    print("# {:<40s} {:>8s} {:>17s} {:>8s} {:>17s} {:>8s} {:>17s}  {:>10s} {:>6s} {:>6s} {:>8s} {:>6s}  same  t<b".format(
        'row', 't ms', 'min .. max', 'r ms', 'min .. max', 'b ms', 'min .. max', 't GB/s i+o', 'peak', 't/r', 'r spread', 'b/t'))
    out = []
    for row in rows:
        res = run_row(row, image, args.reps)
        out.append(res)
        print("  {:<40s} {:8.4f} {:>17s} {:8.4f} {:>17s} {:8.4f} {:>17s}  {:10.1f} {:6.3f} {:6.3f} {:8.3f} {:6.2f}  {:<4s}  {}".format(
            res['row'], res['ms_t'], '{:.4f} .. {:.4f}'.format(*res['ms_t_min_max']), res['ms_r'],
            '{:.4f} .. {:.4f}'.format(*res['ms_r_min_max']), res['ms_b'], '{:.3f} .. {:.3f}'.format(*res['ms_b_min_max']),
            res['GBs_t_moved'], res['t_share_of_hbm_peak'], res['t_over_r'], res['r_spread'], res['b_over_t'],
            'yes' if res['same_bytes_as_decode_encode'] else 'NO',
            'yes' if res['below_the_loop_beyond_its_spread'] else 'NO'))
        sys.stdout.flush()
    for res in out:
        print(json.dumps(res))
    ok = all(r['same_bytes_as_decode_encode'] for r in out)
    return 0 if ok and out[0]['below_the_loop_beyond_its_spread'] else 1


if __name__ == '__main__':
    sys.exit(main())
