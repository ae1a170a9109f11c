#!/usr/bin/env python3
"""Records, per launch shape, the note bb_last_kernel() leaves (kernel, template
arguments, grid, work-item geometry) and the SHA-256 of the output bytes:
tests/golden/launch_notes.json, replayed by tests/test_launch_notes_gpu.py.

Run ONCE on an MI355X with the product library, at the commit whose launches are the
expectation (the parent of a change to the host dispatch).  The shapes are the
smallest at which each work split, grid cap and dispatch branch can still differ;
three size-triggered choices (the 2-bit 64 GiB gather rule, the 16 GiB stripe rule and
the VDIF 8-bit 20 GiB rule without its knob) are out of reach of a test.

    python oracle/gen_golden_launch_notes.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import launch_replay                                                # noqa: E402

VDIF, MARK5B, INT = 0, 1, 2
CASES = []


def case(id_, op, tune=None, **args):
    c = {'id': id_, 'op': op, 'args': args}
    if tune:
        c['tune'] = tune
    CASES.append(c)


# ---- contiguous output ---------------------------------------------------------------------
FLAT = [('vdif1', VDIF, 1), ('vdif2', VDIF, 2), ('vdif4', VDIF, 4), ('vdif8', VDIF, 8), ('int8', INT, 8)]
for name, coder, bps in FLAT:
    for pn in (64, 8000, 10000, 8192):
        for index in (False, True):
            # (the 10000-byte payload of 2-bit samples is the Mark 5B frame)
            c = MARK5B if (bps == 2 and pn == 10000) else coder
            case('flat {} payload {} x 64{}'.format(name, pn, ' indexed' if index else ''), 'decode',
                 coder=c, bps=bps, payload=pn, nframes=64, index=index)
            if name == 'vdif8':
                case('flat vdif8 staged payload {} x 64{}'.format(pn, ' indexed' if index else ''), 'decode',
                     tune={'VDIF8_LDS_GIB': 0}, coder=coder, bps=bps, payload=pn, nframes=64, index=index)
    # 512 work items: the striped work order engages
    case('flat {} payload 1024 x 512 indexed'.format(name), 'decode', coder=coder, bps=bps, payload=1024, nframes=512,
         index=True)
    pn = 8000 if bps > 1 else 2000
    case('flat {} payload {} x 512'.format(name, pn), 'decode', coder=coder, bps=bps, payload=pn, nframes=512, index=False)

# ---- thread interleave ---------------------------------------------------------------------
for nslot, chunk, pn, nframes in ((8, 1, 8000, 12), (8, 2, 8000, 12), (8, 4, 8000, 12), (8, 32, 8000, 12), (2, 64, 8000, 12),
                                  (5, 32, 8000, 12), (16, 64, 8000, 12), (100, 4, 2000, 6)):
    case('interleave 2-bit {} slots x chunk {} indexed'.format(nslot, chunk), 'decode', coder=VDIF, bps=2, payload=pn,
         nframes=nframes, nslot=nslot, chunk=chunk, index=True, complex=chunk >= 2)
for name, coder, bps in (('vdif1', VDIF, 1), ('vdif4', VDIF, 4), ('vdif8', VDIF, 8), ('int8', INT, 8)):
    for chunk in (4, 32):
        case('interleave {} 8 slots x chunk {} indexed'.format(name, chunk), 'decode', coder=coder, bps=bps, payload=8000,
             nframes=12, nslot=8, chunk=chunk, index=True, complex=True)
for chunk in (4, 2):
    case('interleave 2-bit 8 slots x chunk {} fixed stride'.format(chunk), 'decode', coder=VDIF, bps=2, payload=8000,
         nframes=12, nslot=8, chunk=chunk, index=False, complex=True)
# (more slots than the gather stages in its 48 KiB: rows of whole float4 go to k_decode_rows_pipe, narrower ones to the plain kernel)
case('interleave 2-bit 100 slots x chunk 2 indexed', 'decode', coder=VDIF, bps=2, payload=2000, nframes=6, nslot=100, chunk=2,
     index=True, complex=True)
case('interleave 2-bit 8 slots x chunk 32 fixed stride', 'decode', coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8,
     chunk=32, index=False, complex=True)
case('interleave 2-bit 8 slots x chunk 4 x 512 sets indexed', 'decode', coder=VDIF, bps=2, payload=1024, nframes=512, nslot=8,
     chunk=4, index=True, complex=True)
case('interleave 2-bit 8 slots x chunk 32 x 512 sets indexed', 'decode', coder=VDIF, bps=2, payload=1024, nframes=512,
     nslot=8, chunk=32, index=True, complex=True)

# ---- 16-bit output ----------------------------------------------------------------------------
for out in ('f16', 'bf16'):
    for bps in (1, 2):
        for pn in (64, 8000, 10000):
            for index in (False, True):
                case('{} flat {}-bit payload {} x 64{}'.format(out, bps, pn, ' indexed' if index else ''), 'decode',
                     coder=VDIF, bps=bps, payload=pn, nframes=64, index=index, out=out)
    case('{} flat 2-bit payload 1024 x 512 indexed'.format(out), 'decode', coder=VDIF, bps=2, payload=1024, nframes=512,
         index=True, out=out)
    for index in (False, True):
        case('{} interleave 2-bit 8 slots x chunk 4{}'.format(out, ' indexed' if index else ''), 'decode', coder=VDIF, bps=2,
             payload=8000, nframes=12, nslot=8, chunk=4, index=index, complex=True, out=out)
    case('{} interleave 8-bit 5 slots x chunk 32 indexed'.format(out), 'decode', coder=VDIF, bps=8, payload=8000, nframes=12,
         nslot=5, chunk=32, index=True, complex=True, out=out)

# ---- channel subsets ----------------------------------------------------------------------------
case('select keep 1 of 16, 8 slots (pick)', 'decode', coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=16,
     index=True, within=[5])
case('select keep 2 of 16 complex, 8 slots (pick)', 'decode', coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=32,
     index=True, complex=True, within=[6, 7, 24, 25])
case('select keep 8 of 16, 8 slots', 'decode', coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=16, index=True,
     within=[0, 2, 3, 5, 8, 9, 14, 15])
case('select keep 8 of 16, 8 slots, output off the 16-byte grid', 'decode', coder=VDIF, bps=2, payload=8000, nframes=12,
     nslot=8, chunk=16, index=True, within=[0, 2, 3, 5, 8, 9, 14, 15], out_offset=1)
case('select keep 3 of 8, 1 slot, 10000-byte payload', 'decode', coder=MARK5B, bps=2, payload=10000, nframes=12, nslot=1,
     chunk=8, index=True, within=[1, 4, 6])
case('select keep 4 of 16 int8, 2 slots', 'decode', coder=INT, bps=8, payload=8192, nframes=12, nslot=2, chunk=16, index=True,
     within=[1, 4, 6, 15])

# ---- Mark 4 ------------------------------------------------------------------------------------------
for ntrack in (16, 32, 64):
    for widen in (1, 0):
        case('mark4 {} tracks widen {}'.format(ntrack, widen), 'mark4', tune={'M4_WIDEN': widen}, ntrack=ntrack, nwords=20000,
             fill_words=160, nframes=8)
        case('mark4 {} tracks widen {} select'.format(ntrack, widen), 'mark4', tune={'M4_WIDEN': widen}, ntrack=ntrack,
             nwords=20000, fill_words=160, nframes=8, nout=ntrack // 8)
case('mark4 32 tracks, 1999 words (not widened)', 'mark4', ntrack=32, nwords=1999, nframes=8)
case('mark4 32 tracks, 1999 words, select 3 (scalar stores)', 'mark4', ntrack=32, nwords=1999, nframes=8, nout=3)
case('mark4 64 tracks x 512 frames', 'mark4', ntrack=64, nwords=600, nframes=512)

# ---- int8 transposes (the geometries of tests/test_bytefmt_gpu.py) -------------------------------------
for layout, npol, nchan, T, head in ((0, 2, 64, 1024, 32), (1, 2, 64, 1024, 16), (2, 2, 64, 300, 16), (0, 2, 12, 1100, 16),
                                     (1, 1, 10, 1280, 16), (2, 2, 28, 700, 16)):
    unit = 8 // npol if layout == 0 else (8 if layout == 1 else 1)
    for lo, hi in ((0, T), (unit * 2, T - 5)):
        case('xpose layout {} {} pol {} chan {} times [{}, {})'.format(layout, npol, nchan, T, lo, hi), 'tiled', layout=layout,
             npol=npol, nchan=nchan, ntime=T, head=head, nframes=3, t_lo=lo, t_hi=hi)
LIST20 = [151, 3, 77, 12, 90, 41, 8, 133, 60, 21, 5, 99, 142, 30, 64, 17, 110, 2, 58, 86]
for layout in (0, 1, 2):
    # a channel list: k_decode_i8_tf_pick for time-first blocks, k_decode_i8_xpose otherwise
    case('channel list layout {}'.format(layout), 'tiled', layout=layout, npol=2, nchan=20, ntime=512, head=32, nframes=3,
         t_lo=8, t_hi=504, nchan_stored=160, npol_stored=2, chan_map=LIST20, pad16=False)
    case('channel list, one polarisation, layout {}'.format(layout), 'tiled', layout=layout, npol=1, nchan=20, ntime=512,
         head=32, nframes=3, t_lo=0, t_hi=512, nchan_stored=160, npol_stored=2, pol_first=1, chan_map=LIST20, pad16=False)
for stage in (1, 0):
    for layout, npol, nchan, T, head in ((0, 2, 64, 300, 16), (0, 1, 5, 77, 16), (1, 2, 70, 768, 18), (1, 4, 9, 512, 6),
                                         (2, 2, 100, 130, 18), (2, 4, 7, 33, 16)):
        for lo, hi in ((0, T), (3, T - 5)):
            case('general layout {} {} pol {} chan {} times [{}, {}) stage {}'.format(layout, npol, nchan, T, lo, hi, stage),
                 'tiled', tune={'TILED_STAGE': stage}, layout=layout, npol=npol, nchan=nchan, ntime=T, head=head, nframes=3,
                 t_lo=lo, t_hi=hi, pad16=False, index=(lo == 3))
for layout in (0, 1, 2):
    case('xpose switched off, layout {}'.format(layout), 'tiled', tune={'XPOSE': 0}, layout=layout, npol=2, nchan=64, ntime=512,
         head=16, nframes=3, t_lo=0, t_hi=512)

# ---- copies and encoders -----------------------------------------------------------------------------------
case('copy 16-byte aligned', 'copy', nframes=7, n=160000, src0=4096, stride=164096)
case('copy 4-byte aligned', 'copy', nframes=5, n=20004, src0=12, stride=20020)
case('copy x 600 runs', 'copy', nframes=600, n=16400, src0=64, stride=16464)
for coder, bps in ((VDIF, 2), (VDIF, 4), (MARK5B, 1), (INT, 8)):
    case('encode_flat coder {} {}-bit'.format(coder, bps), 'encode_flat', coder=coder, bps=bps, nelem=(1 << 20) + 4096 + 64)
    case('encode_flat coder {} {}-bit, short'.format(coder, bps), 'encode_flat', coder=coder, bps=bps, nelem=64)
for ntrack in (16, 32, 64):
    case('encode_mark4 {} tracks'.format(ntrack), 'encode_mark4', ntrack=ntrack, nwords=20000)

# ---- BB_TUNE_BLOCKS = 7: the cap, and workgroups that loop over their items ----------------------------------
B7 = {'BLOCKS': 7}
case('7 blocks: gather', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=4, index=True,
     complex=True)
case('7 blocks: rows_pipe', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=32, index=True,
     complex=True)
for name, coder, bps in FLAT:
    case('7 blocks: flat {}'.format(name), 'decode', tune=B7, coder=coder, bps=bps, payload=8000, nframes=64, index=True)
case('7 blocks: flat vdif8 staged', 'decode', tune=dict(B7, VDIF8_LDS_GIB=0), coder=VDIF, bps=8, payload=8000, nframes=64,
     index=True)
case('7 blocks: plain kernel, interleave without an index', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=12,
     nslot=8, chunk=4, index=False, complex=True)
case('7 blocks: f16 flat', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=64, index=True, out='f16')
case('7 blocks: bf16 interleave', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=4, index=True,
     complex=True, out='bf16')
case('7 blocks: pick', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=16, index=True, within=[5])
case('7 blocks: gather_select', 'decode', tune=B7, coder=VDIF, bps=2, payload=8000, nframes=12, nslot=8, chunk=16, index=True,
     within=[0, 2, 3, 5, 8, 9, 14, 15])
case('7 blocks: mark4', 'mark4', tune=B7, ntrack=64, nwords=20000, fill_words=160, nframes=8)
case('7 blocks: mark4 32 tracks widened', 'mark4', tune=B7, ntrack=32, nwords=20000, fill_words=160, nframes=8)
case('7 blocks: mark4 select (ignores the knob)', 'mark4', tune=B7, ntrack=64, nwords=20000, fill_words=160, nframes=8, nout=8)
case('7 blocks: xpose', 'tiled', tune=B7, layout=0, npol=2, nchan=64, ntime=1024, head=32, nframes=3, t_lo=0, t_hi=1024)
case('7 blocks: tf_pick', 'tiled', tune=B7, layout=2, npol=2, nchan=20, ntime=512, head=32, nframes=3, t_lo=8, t_hi=504,
     nchan_stored=160, npol_stored=2, chan_map=LIST20, pad16=False)
case('7 blocks: stage', 'tiled', tune=B7, layout=1, npol=2, nchan=70, ntime=768, head=18, nframes=3, t_lo=0, t_hi=768,
     pad16=False)
case('7 blocks: tiled', 'tiled', tune=B7, layout=0, npol=2, nchan=64, ntime=300, head=16, nframes=3, t_lo=3, t_hi=295,
     pad16=False)
case('7 blocks: copy', 'copy', tune=B7, nframes=7, n=160000, src0=4096, stride=164096)
case('7 blocks: encode_flat', 'encode_flat', tune=B7, coder=VDIF, bps=2, nelem=(1 << 20) + 4096 + 64)
case('7 blocks: encode_mark4', 'encode_mark4', tune=B7, ntrack=32, nwords=20000)


def main():
    import torch
    from baseband_amd import _lib
    assert torch.cuda.is_available() and not _lib.EXPERIMENTS, "record this table on a GPU, with the product library"
    ids = [c['id'] for c in CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    for c in CASES:
        c['note'], c['sha256'] = launch_replay.run(c)
        print(c['id'], '->', c['note'], flush=True)
    out_dir = os.environ.get('BB_GOLDEN_OUT', os.path.join(ROOT, 'tests', 'golden'))
    path = os.path.join(out_dir, 'launch_notes.json')
    with open(path, 'w') as f:
        f.write('{"cases": [\n' + ',\n'.join(json.dumps(c, sort_keys=True) for c in CASES) + '\n]}\n')
    print("{} launches, {} distinct notes -> {}".format(len(CASES), len({c['note'] for c in CASES}), path))


if __name__ == '__main__':
    main()
