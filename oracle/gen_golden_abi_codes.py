#!/usr/bin/env python3
"""Records what the C ABI's argument checks answer: tests/golden/abi_return_codes.json,
replayed by tests/test_abi_codes.py.

Run ONCE, at the commit whose answers are the expectation (the parent of a change to
the host dispatch; last: the parent of the change that moved the packed-byte entries
bb_count_states, bb_count_states_bins, bb_repack_frames and bb_requant_frames into
csrc/bb_packed.inc, which added the rows of bb_requant_frames), on a
machine WITHOUT a device: every check runs before the first HIP call, so a call with
one fault answers its code there and a call without a fault stops at BB_EIO.  Device
addresses are made up; nothing follows them on the host.  The decode, encode, scan and
window entries have single-fault calls only; the packed-byte entries also have one call
per pair of checks that answer different codes, which holds their ORDER in place.  Only
calls that answer something other than BB_EIO are recorded -- asserted below.

    python oracle/gen_golden_abi_codes.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import abi_replay                                                   # noqa: E402

# made-up device addresses, 4 KiB aligned
BUF, OUT, SRC, RECS, OFFS, CNT, NBAD, WITHIN, SLOTMAP, IN, BADTR, CMAP = (0x7f0000001000 + k * 0x100000 for k in range(12))
EVENT, SIDE = 0x7e0000001000, 0x7e0000002000                        # event / stream handles (never used before a check fails)
PER_GRID = 0x7fffffff                                               # most workgroups of a launch

CASES = []


def S(name, **f):
    return {'struct': name, 'f': f}


def entry(fn, names, base):
    """-> add(label, **changes): one recorded call of `fn`, the valid call `base` with
    `changes`; ``p__field=v`` changes a field of the parameter block named p."""
    def add(label, **changes):
        args = {k: (dict(v, f=dict(v['f'])) if isinstance(v, dict) and 'f' in v else v) for k, v in base.items()}
        for k, v in changes.items():
            if '__' in k:
                blk, field = k.split('__', 1)
                args[blk]['f'][field] = v
            else:
                assert k in args, k
                args[k] = v
        CASES.append({'id': '{}:{}'.format(fn, label), 'fn': fn, 'args': [args[n] for n in names]})
    return add


def dec(out_type=0, **f):
    d = dict(coder=0, bps=2, chunk=1, nslot=1, payload_nbytes=64, src0=0, src_stride=64, out_type=out_type)
    d.update(f)
    return S('DecodeParams', **d)


# ---- bb_decode_frames, every output type -------------------------------------------
DEC = ['d_buf', 'buf_nbytes', 'd_src', 'nframes', 'p', 'd_out', 'out_elems', 'stream']
for t, tn in ((0, 'f32'), (1, 'f16'), (2, 'bf16')):
    add = entry('bb_decode_frames', DEC, dict(d_buf=BUF, buf_nbytes=256, d_src=None, nframes=4, p=dec(t), d_out=OUT,
                                              out_elems=1024, stream=None))
    if t == 0:
        add('null parameter block', p=None)
    add(tn + ' null buffer', d_buf=None)
    add(tn + ' null output', d_out=None)
    add(tn + ' buffer not 4-byte aligned', d_buf=BUF + 2)
    add(tn + ' output not 16-byte aligned (+4)', d_out=OUT + 4)
    add(tn + ' output not 16-byte aligned (+8)', d_out=OUT + 8)
    add(tn + ' output one element short', out_elems=1023)
    add(tn + ' source range one byte past the end', buf_nbytes=255)
    add(tn + ' negative src0', p__src0=-4)
    add(tn + ' misaligned src0', p__src0=2, buf_nbytes=512)
    add(tn + ' negative src_stride', p__src_stride=-64)
    add(tn + ' misaligned src_stride', p__src_stride=66, buf_nbytes=512)
    add(tn + ' Mark 5B has no 4-bit coder', p__coder=1, p__bps=4)
    add(tn + ' 3 bits per sample', p__bps=3)
    add(tn + ' INT has no 2-bit coder', p__coder=2)
    add(tn + ' unknown coder', p__coder=7)
    add(tn + ' payload not whole dwords', p__payload_nbytes=62)
    add(tn + ' empty payload', p__payload_nbytes=0)
    add(tn + ' nslot 0', p__nslot=0)
    add(tn + ' chunk 0', p__chunk=0)
    add(tn + ' nframes 0', nframes=0)
    add(tn + ' nframes 0, null buffers', nframes=0, d_buf=None, d_out=None, out_elems=0, buf_nbytes=0)
    add(tn + ' nframes 0, payload not whole dwords', nframes=0, p__payload_nbytes=62)
    add(tn + ' nframes 0, nslot 0', nframes=0, p__nslot=0)
    add(tn + ' nframes 0, chunk 0', nframes=0, p__chunk=0)
    add(tn + ' nframes 0, unsupported coder', nframes=0, p__coder=1, p__bps=4)
    # thread interleave, through an index (no source range to check)
    addi = entry('bb_decode_frames', DEC, dict(d_buf=BUF, buf_nbytes=1 << 20, d_src=SRC, nframes=4,
                                               p=dec(t, chunk=4, nslot=2, payload_nbytes=96), d_out=OUT,
                                               out_elems=1 << 24, stream=None))
    addi(tn + ' chunk not a power of two with two slots', p__chunk=24)
    addi(tn + ' payload not whole rows', p__bps=8, p__chunk=64)
    addi(tn + ' interleave: output one element short', out_elems=4 * 2 * 384 - 1)
    addi(tn + ' nframes 0, chunk not a power of two with two slots', nframes=0, p__chunk=24)
    if t:
        addi(tn + ' 4096 slots', p__nslot=4096)
        addi(tn + ' 2049 slots', p__nslot=2049)
add = entry('bb_decode_frames', DEC, dict(d_buf=BUF, buf_nbytes=256, d_src=None, nframes=4, p=dec(0), d_out=OUT,
                                          out_elems=1024, stream=None))
add('out_type 3', p__out_type=3)
add('out_type -1', p__out_type=-1)
add('out_type 3, nframes 0', p__out_type=3, nframes=0)

# ---- bb_decode_frames_select --------------------------------------------------------
SEL = ['d_buf', 'buf_nbytes', 'd_src', 'nframes', 'p', 'd_within', 'nwithin', 'd_out', 'out_elems', 'stream']
add = entry('bb_decode_frames_select', SEL,
            dict(d_buf=BUF, buf_nbytes=1 << 20, d_src=SRC, nframes=2, p=dec(0, chunk=32, nslot=8, payload_nbytes=8000),
                 d_within=WITHIN, nwithin=4, d_out=OUT, out_elems=2 * 1000 * 8 * 4, stream=None))
add('null parameter block', p=None)
add('f16 with a channel subset', p__out_type=1)
add('bf16 with a channel subset', p__out_type=2)
add('out_type 3', p__out_type=3)
add('3 bits per sample', p__bps=3)
add('nslot 0', p__nslot=0)
add('chunk 0', p__chunk=0)
add('nwithin 0', nwithin=0)
add('nwithin 4097', nwithin=4097)
add('payload not whole dwords', p__payload_nbytes=62)
add('chunk not a power of two', p__chunk=24)
add('payload not whole rows', p__chunk=64, p__payload_nbytes=8)
add('more slots than the staging takes', p__nslot=512)
add('nframes 0', nframes=0)
add('null buffer', d_buf=None)
add('null output', d_out=None)
add('null index', d_src=None)
add('null selection', d_within=None)
add('buffer not 4-byte aligned', d_buf=BUF + 2)
add('output not 4-byte aligned', d_out=OUT + 2)
add('output one element short', out_elems=2 * 1000 * 8 * 4 - 1)

# ---- bb_copy_frames ------------------------------------------------------------------
add = entry('bb_copy_frames', ['d_buf', 'buf_nbytes', 'nframes', 'n', 'src0', 'src_stride', 'd_out', 'out_nbytes', 'stream'],
            dict(d_buf=BUF, buf_nbytes=256, nframes=4, n=64, src0=0, src_stride=64, d_out=OUT, out_nbytes=256, stream=None))
add('nframes 0', nframes=0)
add('no bytes per frame', n=0)
add('null buffer', d_buf=None)
add('null output', d_out=None)
add('bytes per frame not whole dwords', n=62, src_stride=64)
add('misaligned src0', src0=2, buf_nbytes=512)
add('misaligned src_stride', src_stride=66, buf_nbytes=512)
add('negative src0', src0=-4)
add('negative src_stride', src_stride=-64)
add('buffer not 4-byte aligned', d_buf=BUF + 2)
add('output not 4-byte aligned', d_out=OUT + 2)
add('overlapping runs', src_stride=32)
add('output one byte short', out_nbytes=255)
add('source range one byte past the end', buf_nbytes=255)

# ---- bb_decode_mark4 / bb_decode_mark4_select ----------------------------------------
SIGN, MAG = [2 * j for j in range(16)], [2 * j + 1 for j in range(16)]


def m4(**f):
    d = dict(ntrack=32, out_type=0, nwords=64, fill_words=0, src0=0, src_stride=256, sign_bit=list(SIGN), mag_bit=list(MAG))
    d.update(f)
    return S('Mark4DecodeParams', **d)


for fn, names, extra, oalign in (('bb_decode_mark4', DEC, {}, 4),
                                 ('bb_decode_mark4_select',
                                  ['d_buf', 'buf_nbytes', 'd_src', 'nframes', 'p', 'nout', 'd_out', 'out_elems', 'stream'],
                                  {'nout': 16}, 2)):
    add = entry(fn, names, dict(d_buf=BUF, buf_nbytes=512, d_src=None, nframes=2, p=m4(), d_out=OUT, out_elems=2048,
                                stream=None, **extra))
    add('null parameter block', p=None)
    add('24 tracks', p__ntrack=24)
    add('nframes 0', nframes=0)
    add('f16', p__out_type=1)
    add('bf16', p__out_type=2)
    add('out_type 3', p__out_type=3)
    add('null buffer', d_buf=None)
    add('null output', d_out=None)
    add('no words', p__nwords=0)
    add('more fill words than words', p__fill_words=65)
    add('buffer not 8-byte aligned', d_buf=BUF + 4)
    add('output misaligned', d_out=OUT + oalign)
    add('sign bit past the word', p__sign_bit=[32] + SIGN[1:])
    add('magnitude bit past the word', p__mag_bit=MAG[:15] + [40])
    add('output one element short', out_elems=2047)
    add('source range one byte past the end', buf_nbytes=511)
    add('negative src0', p__src0=-4)
    add('src0 not whole words', p__src0=2, buf_nbytes=1024)
    add('src_stride not whole words', p__src_stride=258, buf_nbytes=1024)
    add('negative src_stride', p__src_stride=-256)
    if extra:
        add('nout 0', nout=0)
        add('nout 33', nout=33)
add = entry('bb_decode_mark4', DEC, dict(d_buf=BUF, buf_nbytes=1024, d_src=None, nframes=2,
                                         p=m4(ntrack=64, src_stride=512, sign_bit=[2 * j for j in range(32)],
                                              mag_bit=[2 * j + 1 for j in range(32)]),
                                         d_out=OUT, out_elems=4096, stream=None))
add('64 tracks: src0 not whole words', p__src0=4, buf_nbytes=2048)
add('64 tracks: src_stride not whole words', p__src_stride=516, buf_nbytes=2048)
add = entry('bb_decode_mark4', DEC, dict(d_buf=BUF, buf_nbytes=256, d_src=None, nframes=2,
                                         p=m4(ntrack=16, src_stride=128, sign_bit=[2 * j for j in range(8)],
                                              mag_bit=[2 * j + 1 for j in range(8)]),
                                         d_out=OUT, out_elems=1024, stream=None))
add('16 tracks: src0 not whole words', p__src0=1, buf_nbytes=512)
add('16 tracks: source range one byte past the end', buf_nbytes=255)

# ---- bb_decode_i8_tiled -----------------------------------------------------------------
def tiled(**f):
    d = dict(layout=0, npol=2, nchan=4, nchan_stored=0, ntime=16, t_lo=0, t_hi=16, src0=0, src_stride=256,
             npol_stored=0, pol_first=0, d_chan_map=None)
    d.update(f)
    return S('TiledParams', **d)


add = entry('bb_decode_i8_tiled', DEC, dict(d_buf=BUF, buf_nbytes=512, d_src=None, nframes=2, p=tiled(), d_out=OUT,
                                            out_elems=512, stream=None))
add('null parameter block', p=None)
add('layout 3', p__layout=3)
add('npol 0', p__npol=0)
add('nchan 0', p__nchan=0)
add('t_hi past ntime', p__t_hi=17)
add('t_lo past t_hi', p__t_lo=12, p__t_hi=8)
add('MKBF heap not 256 times', p__layout=1)
add('nframes 0', nframes=0)
add('no rows', p__t_lo=8, p__t_hi=8)
add('null buffer', d_buf=None)
add('null output', d_out=None)
add('buffer not 2-byte aligned', d_buf=BUF + 1)
add('output not 16-byte aligned', d_out=OUT + 4)
add('output one element short', out_elems=511)
add('negative nchan_stored', p__nchan_stored=-1)
add('fewer stored channels than decoded, no map', p__nchan_stored=2)
add('negative npol_stored', p__npol_stored=-1)
add('negative pol_first', p__pol_first=-1)
add('polarisations past the stored ones', p__pol_first=1)
add('channel map without nchan_stored', p__d_chan_map=CMAP)
add('negative src0', p__src0=-2)
add('odd src0', p__src0=1, buf_nbytes=1024)
add('odd src_stride', p__src_stride=257, buf_nbytes=1024)
add('negative src_stride', p__src_stride=-256)
add('source range one byte past the end', buf_nbytes=511)
add('selection the fast form does not take', nframes=1, p__nchan=3, p__nchan_stored=8, p__d_chan_map=CMAP,
    out_elems=16 * 2 * 3 * 2)

# ---- encoders ----------------------------------------------------------------------------
add = entry('bb_encode_flat', ['d_in', 'nelem', 'coder', 'bps', 'd_out', 'out_nbytes', 'stream'],
            dict(d_in=IN, nelem=64, coder=0, bps=2, d_out=OUT, out_nbytes=16, stream=None))
add('Mark 5B has no 4-bit coder', coder=1, bps=4, out_nbytes=32)
add('3 bits per sample', bps=3)
add('nelem 0', nelem=0)
add('null input', d_in=None)
add('null output', d_out=None)
add('not whole quads', nelem=62)
add('not whole bytes', nelem=4, bps=1)
add('input not 16-byte aligned', d_in=IN + 4)
add('output not 4-byte aligned', d_out=OUT + 2)
add('output one byte short', out_nbytes=15)
add = entry('bb_encode_mark4', ['d_in', 'nwords', 'ntrack', 'sign', 'mag', 'd_out', 'out_nbytes', 'stream'],
            dict(d_in=IN, nwords=16, ntrack=32, sign={'u8': SIGN}, mag={'u8': MAG}, d_out=OUT, out_nbytes=64, stream=None))
add('24 tracks', ntrack=24)
add('nwords 0', nwords=0)
add('null input', d_in=None)
add('null output', d_out=None)
add('null sign map', sign=None)
add('null magnitude map', mag=None)
add('input not 16-byte aligned', d_in=IN + 4)
add('output not 8-byte aligned', d_out=OUT + 4)
add('output one byte short', out_nbytes=63)
add('sign bit past the word', sign={'u8': SIGN[:3] + [32] + SIGN[4:]})

# ---- scans, searches, verification, index -------------------------------------------------
def vscan(**f):
    d = dict(first_offset=0, frame_nbytes=96, header_nbytes=32, ref_seconds=0, ref_frame_nr=0, frame_rate=100, set_nframes=0)
    d.update(f)
    return S('VDIFScanParams', **d)


add = entry('bb_vdif_scan', ['d_buf', 'nbytes', 'p', 'd_recs', 'nframes', 'stream'],
            dict(d_buf=BUF, nbytes=384, p=vscan(), d_recs=RECS, nframes=4, stream=None))
add('nframes 0', nframes=0)
add('null buffer', d_buf=None)
add('null parameter block', p=None)
add('null records', d_recs=None)
add('24-byte header', p__header_nbytes=24)
add('frame shorter than its header', p__frame_nbytes=16)
add('frame not whole 8 bytes', p__frame_nbytes=100)
add('misaligned first_offset', p__first_offset=2)
add('buffer not 4-byte aligned', d_buf=BUF + 2)
add('one frame more than a grid takes', nframes=PER_GRID * 32 + 1)
add = entry('bb_vdif_scan_at', ['d_buf', 'nbytes', 'p', 'd_offsets', 'nframes', 'd_recs', 'stream'],
            dict(d_buf=BUF, nbytes=384, p=vscan(), d_offsets=OFFS, nframes=4, d_recs=RECS, stream=None))
add('nframes 0', nframes=0)
add('null buffer', d_buf=None)
add('null parameter block', p=None)
add('null offsets', d_offsets=None)
add('null records', d_recs=None)
add('24-byte header', p__header_nbytes=24)
add('buffer not 4-byte aligned', d_buf=BUF + 2)
add('one frame more than a grid takes', nframes=PER_GRID * 256 + 1)
add = entry('bb_vdif_locate', ['d_buf', 'nbytes', 'p', 'd_offsets', 'cap', 'd_count', 'stream'],
            dict(d_buf=BUF, nbytes=384, p=vscan(), d_offsets=OFFS, cap=16, d_count=CNT, stream=None))
add('null buffer', d_buf=None)
add('null parameter block', p=None)
add('null offsets', d_offsets=None)
add('null count', d_count=None)
add('24-byte header', p__header_nbytes=24)
add('frame shorter than its header', p__frame_nbytes=16)
add('buffer not 16-byte aligned', d_buf=BUF + 8)
add('buffer shorter than a frame', nbytes=95)

m5scan = S('Mark5BScanParams', first_offset=0, ref_seconds=0, ref_frame_nr=0, frame_rate=100, by_position=0)
add = entry('bb_mark5b_scan', ['d_buf', 'nbytes', 'p', 'd_recs', 'nframes', 'stream'],
            dict(d_buf=BUF, nbytes=40064, p=m5scan, d_recs=RECS, nframes=4, stream=None))
add('nframes 0', nframes=0)
add('null buffer', d_buf=None)
add('null parameter block', p=None)
add('null records', d_recs=None)
add('misaligned first_offset', p__first_offset=2)
add('buffer not 4-byte aligned', d_buf=BUF + 2)
add('one frame more than a grid takes', nframes=PER_GRID * 4 + 1)
add = entry('bb_mark5b_scan_at', ['d_buf', 'nbytes', 'p', 'd_offsets', 'nframes', 'd_recs', 'stream'],
            dict(d_buf=BUF, nbytes=40064, p=m5scan, d_offsets=OFFS, nframes=4, d_recs=RECS, stream=None))
add('nframes 0', nframes=0)
add('null offsets', d_offsets=None)
add('null buffer', d_buf=None)
add('null records', d_recs=None)
add('buffer not 4-byte aligned', d_buf=BUF + 2)
add('one frame more than a grid takes', nframes=PER_GRID * 4 + 1)
add = entry('bb_mark5b_locate', ['d_buf', 'nbytes', 'd_offsets', 'cap', 'd_count', 'stream'],
            dict(d_buf=BUF, nbytes=40064, d_offsets=OFFS, cap=16, d_count=CNT, stream=None))
add('null buffer', d_buf=None)
add('null offsets', d_offsets=None)
add('null count', d_count=None)
add('buffer not 16-byte aligned', d_buf=BUF + 8)
add('buffer shorter than a frame', nbytes=10015)
add = entry('bb_mark5b_locate_stream', ['d_buf', 'nbytes', 'w1p', 'w1m', 'd_offsets', 'cap', 'd_count', 'stream'],
            dict(d_buf=BUF, nbytes=40064, w1p=0, w1m=0, d_offsets=OFFS, cap=16, d_count=CNT, stream=None))
add('null buffer', d_buf=None)
add('buffer not 16-byte aligned', d_buf=BUF + 4)
add('buffer shorter than a frame', nbytes=10015)

m4scan = S('Mark4ScanParams', first_offset=0, ntrack=32, ref_year=2020, ref_qms=0, frame_qms=10, by_position=0)
add = entry('bb_mark4_scan', ['d_buf', 'nbytes', 'p', 'd_recs', 'nframes', 'stream'],
            dict(d_buf=BUF, nbytes=320000, p=m4scan, d_recs=RECS, nframes=4, stream=None))
add('nframes 0', nframes=0)
add('null buffer', d_buf=None)
add('null parameter block', p=None)
add('null records', d_recs=None)
add('24 tracks', p__ntrack=24)
add('first_offset not whole words', p__first_offset=2)
add('buffer not 8-byte aligned', d_buf=BUF + 4)
add('negative frame_qms', p__frame_qms=-1)
add('one frame more than a grid takes', nframes=PER_GRID * 4 + 1)
add = entry('bb_mark4_scan_at', ['d_buf', 'nbytes', 'p', 'd_offsets', 'nframes', 'd_recs', 'stream'],
            dict(d_buf=BUF, nbytes=320000, p=m4scan, d_offsets=OFFS, nframes=4, d_recs=RECS, stream=None))
add('nframes 0', nframes=0)
add('null offsets', d_offsets=None)
add('null buffer', d_buf=None)
add('24 tracks', p__ntrack=24)
add('buffer not 8-byte aligned', d_buf=BUF + 4)
add('one frame more than a grid takes', nframes=PER_GRID * 4 + 1)
add = entry('bb_mark4_locate', ['d_buf', 'nbytes', 'ntrack', 'd_offsets', 'cap', 'd_count', 'stream'],
            dict(d_buf=BUF, nbytes=320000, ntrack=32, d_offsets=OFFS, cap=16, d_count=CNT, stream=None))
add('null buffer', d_buf=None)
add('null offsets', d_offsets=None)
add('null count', d_count=None)
add('24 tracks', ntrack=24)
add('buffer not 16-byte aligned', d_buf=BUF + 8)
add('buffer shorter than a frame', nbytes=79999)
add = entry('bb_mark4_header_crc', ['d_buf', 'nbytes', 'ntrack', 'd_offsets', 'first_offset', 'nframes', 'd_bad', 'stream'],
            dict(d_buf=BUF, nbytes=320000, ntrack=32, d_offsets=None, first_offset=0, nframes=4, d_bad=BADTR, stream=None))
add('nframes 0', nframes=0)
add('null buffer', d_buf=None)
add('null result', d_bad=None)
add('24 tracks', ntrack=24)
add('negative first_offset', first_offset=-4)
add('one frame more than a grid takes', nframes=PER_GRID * 256 + 1)
add = entry('bb_verify_records', ['d_recs', 'nrecs', 'first_index', 'recs_per_index', 'nstrict', 'd_nbad', 'stream'],
            dict(d_recs=RECS, nrecs=4, first_index=0, recs_per_index=1, nstrict=4, d_nbad=NBAD, stream=None))
add('null counter', d_nbad=None)
add('null records', d_recs=None)
add('recs_per_index 0', recs_per_index=0)
add('nrecs 0', nrecs=0)
add('one record more than a grid takes', nrecs=PER_GRID * 256 + 1)
add = entry('bb_build_index', ['d_recs', 'nrecs', 'd_thread_slot', 'nslot', 'd_src', 'nframes_out', 'stream'],
            dict(d_recs=RECS, nrecs=4, d_thread_slot=None, nslot=1, d_src=SRC, nframes_out=0, stream=None))
add('null index', d_src=None)
add('nslot 0', nslot=0)
add('null records', d_recs=None)
add('nrecs 0, no index entries', nrecs=0)
add('one record more than a grid takes', nrecs=PER_GRID * 256 + 1)

# ---- window calls --------------------------------------------------------------------------
VWIN = ['d_buf', 'nbytes', 'scan', 'nframes', 'd_thread_slot', 'nsets', 'dec', 'd_within', 'nwithin', 'd_recs', 'd_src',
        'd_out', 'out_elems', 'recs_per_index', 'nstrict', 'd_nbad', 'verified', 'scan_stream', 'stream']
for t, tn in ((0, 'f32'), (1, 'f16'), (2, 'bf16')):
    add = entry('bb_vdif_read_window', VWIN,
                dict(d_buf=BUF, nbytes=16 * 96, scan=vscan(), nframes=16, d_thread_slot=SLOTMAP, nsets=2,
                     dec=dec(t, chunk=4, nslot=8), d_within=None, nwithin=0, d_recs=RECS, d_src=SRC, d_out=OUT,
                     out_elems=2 * 8 * 256, recs_per_index=8, nstrict=0, d_nbad=None, verified=None, scan_stream=None,
                     stream=None))
    add(tn + ' null scan block', scan=None)
    add(tn + ' null decode block', dec=None)
    add(tn + ' null index', d_src=None)
    add(tn + ' nslot 0', dec__nslot=0)
    add(tn + ' scan_stream without verified', scan_stream=SIDE)
    add(tn + ' null buffer', d_buf=None)
    add(tn + ' null records', d_recs=None)
    add(tn + ' 24-byte header', scan__header_nbytes=24)
    add(tn + ' buffer not 4-byte aligned', d_buf=BUF + 2)
    if t:
        add(tn + ' 4096 slots', dec__nslot=4096)
        add(tn + ' with a channel subset', d_within=WITHIN, nwithin=2)
        add(tn + ' payload not whole dwords', dec__payload_nbytes=62)
        add(tn + ' 3 bits per sample', dec__bps=3)
        add(tn + ' chunk not a power of two', dec__chunk=24, dec__payload_nbytes=96)
    else:
        add('out_type 3', dec__out_type=3)
M5WIN = ['d_buf', 'nbytes', 'scan', 'nframes', 'n', 'dec', 'd_within', 'nwithin', 'd_recs', 'd_src', 'd_out', 'out_elems',
         'nstrict', 'd_nbad', 'verified', 'scan_stream', 'stream']
for t, tn in ((0, 'f32'), (1, 'f16'), (2, 'bf16')):
    add = entry('bb_mark5b_read_window', M5WIN,
                dict(d_buf=BUF, nbytes=40064, scan=m5scan, nframes=4, n=4,
                     dec=dec(t, coder=1, payload_nbytes=10000, src_stride=0), d_within=None, nwithin=0, d_recs=RECS,
                     d_src=SRC, d_out=OUT, out_elems=4 * 40000, nstrict=0, d_nbad=None, verified=None, scan_stream=None,
                     stream=None))
    add(tn + ' null scan block', scan=None)
    add(tn + ' null decode block', dec=None)
    add(tn + ' scan_stream without verified', scan_stream=SIDE)
    add(tn + ' null buffer', d_buf=None)
    add(tn + ' null records', d_recs=None)
    add(tn + ' misaligned first_offset', scan__first_offset=2)
    add(tn + ' nothing to read', nframes=0, n=0)
    if t:
        add(tn + ' with a channel subset', d_within=WITHIN, nwithin=2)
        add(tn + ' 4-bit Mark 5B', dec__bps=4)
    else:
        add('out_type 3', dec__out_type=3)
add = entry('bb_mark4_read_window',
            ['d_buf', 'nbytes', 'scan', 'nframes', 'n', 'dec', 'nout', 'd_recs', 'd_src', 'd_out', 'out_elems', 'nstrict',
             'd_nbad', 'verified', 'scan_stream', 'stream'],
            dict(d_buf=BUF, nbytes=320000, scan=m4scan, nframes=4, n=4, dec=m4(nwords=20000, src_stride=0), nout=0,
                 d_recs=RECS, d_src=SRC, d_out=OUT, out_elems=4 * 20000 * 16, nstrict=0, d_nbad=None, verified=None,
                 scan_stream=None, stream=None))
add('null scan block', scan=None)
add('null decode block', dec=None)
add('scan_stream without verified', scan_stream=SIDE)
add('24 tracks', scan__ntrack=24)
add('null buffer', d_buf=None)
add('null records', d_recs=None)
add('buffer not 8-byte aligned', d_buf=BUF + 4)
add('nothing to read', nframes=0, n=0)
add('nothing to read, selecting', nframes=0, n=0, nout=4)

# ---- the packed-byte entries: statistics, repack and requantize -----------------------------------------
# Single faults as above, and DOUBLE faults: what a reordering of the checks would change
# unseen.  A rule is (statement, label, changes): `statement` names the `if` of the entry
# that answers it.  main() pairs the first rule of every statement with the first rule of
# every other statement that answers another code (one call per pair of statements, not of
# values); pairs whose changes contradict each other are left out, PAIRED_BY_HAND adds the
# ones worth a call of their own.
PAIRED = []                                                         # (fn, names, base, rules)


def rules(fn, names, base, table):
    add = entry(fn, names, base)
    for _, label, changes in table:
        add(label, **changes)
    PAIRED.append((fn, names, base, table))
    return add


def states(**f):
    d = dict(bps=2, chunk=1, nslot=1, reserved=0, payload_nbytes=192, src0=0, src_stride=192, row_lo=0, row_hi=8)
    d.update(f)
    return S('StatesParams', **d)


# 4 frames of 192 bytes: 768 rows of one 2-bit code each; chunk 3 still makes whole rows
STATES_RULES = [
    ('bps', '3 bits per sample', dict(p__bps=3)),
    ('fields', 'reserved set', dict(p__reserved=1)),
    ('fields', 'nslot 0', dict(p__nslot=0)),
    ('fields', 'chunk 0', dict(p__chunk=0)),
    ('pow2', 'chunk not a power of two', dict(p__chunk=3)),
    ('row bits', 'rows of more than 128 bits', dict(p__chunk=128)),
    ('payload', 'payload not whole dwords', dict(p__payload_nbytes=190)),
    ('payload', 'empty payload', dict(p__payload_nbytes=0)),
    ('payload', 'payload above 2^56', dict(p__payload_nbytes=(1 << 56) + 4)),
    ('whole rows', 'payload not whole rows', dict(p__payload_nbytes=196, p__chunk=32)),
    ('row order', 'row_lo past row_hi', dict(p__row_lo=16)),
]
SOURCE_RULES = [
    ('empty', 'no rows', dict(p__row_lo=8)),
    ('empty', 'nframes 0', dict(nframes=0, p__row_hi=0)),
    ('buffer', 'null buffer', dict(d_buf=None)),
    ('buffer', 'buffer not 4-byte aligned', dict(d_buf=BUF + 2)),
    ('stride', 'misaligned src0', dict(p__src0=2)),
    ('stride', 'negative src0', dict(p__src0=-4)),
    ('stride', 'misaligned src_stride', dict(p__src_stride=194)),
    ('stride', 'negative src_stride', dict(p__src_stride=-192)),
    ('source range', 'source range one byte past the end', dict(buf_nbytes=767)),
]
CS = ['d_buf', 'buf_nbytes', 'd_src', 'nframes', 'p', 'd_counts', 'ncounts', 'stream']
add = rules('bb_count_states', CS,
            dict(d_buf=BUF, buf_nbytes=768, d_src=None, nframes=4, p=states(), d_counts=CNT, ncounts=1024, stream=None),
            STATES_RULES + [
                ('counts', 'null counts', dict(d_counts=None)),
                ('counts', 'counts not 8-byte aligned', dict(d_counts=CNT + 4)),
                ('ncounts', 'counts one short', dict(ncounts=3)),
                ('rows overflow', 'more rows than 64 bits count', dict(nframes=1 << 60)),
                ('row range', 'row_hi past the last row', dict(p__row_hi=4 * 768 + 8)),
            ] + SOURCE_RULES + [
                ('work', 'more work items in a frame than 32 bits count', dict(d_src=SRC, p__payload_nbytes=1 << 50)),
            ])
add('null parameter block', p=None)
add('nframes 0, null buffers', nframes=0, p__row_hi=0, d_buf=None, buf_nbytes=0)
add('more workgroups than a grid holds', d_src=SRC, nframes=1 << 40, p__payload_nbytes=1 << 20, p__nslot=32,
    p__row_hi=1 << 62)

CSB = ['d_buf', 'buf_nbytes', 'd_src', 'nframes', 'p', 'bin_rows', 'first_row', 'nbins', 'd_counts', 'ncounts', 'stream']
add = rules('bb_count_states_bins', CSB,
            dict(d_buf=BUF, buf_nbytes=768, d_src=None, nframes=4, p=states(), bin_rows=4, first_row=0, nbins=2,
                 d_counts=CNT, ncounts=1024, stream=None),
            STATES_RULES + [
                ('bin_rows', 'bin_rows 0', dict(bin_rows=0)),
                ('bin_rows', 'bin_rows 2^31', dict(bin_rows=1 << 31)),
                ('bin bytes', 'bins not whole bytes', dict(bin_rows=6)),
                ('counters', 'more counters per bin than a window takes', dict(p__chunk=16, p__bps=8,
                                                                               p__payload_nbytes=64, p__src_stride=64)),
                ('counts', 'null counts', dict(d_counts=None)),
                ('counts', 'counts not 4-byte aligned', dict(d_counts=CNT + 2)),
                ('first_row', 'first_row above 2^56', dict(first_row=(1 << 56) + 8)),
                ('whole bytes', 'first_row not a whole byte', dict(first_row=2)),
                ('whole bytes', 'row_lo not a whole byte', dict(p__row_lo=2)),
                ('whole bytes', 'row_hi not a whole byte', dict(p__row_hi=10)),
                ('ncounts', 'counts one short', dict(ncounts=7)),
                ('ncounts', 'more counters than 64 bits count', dict(nbins=1 << 62)),
                ('rows overflow', 'more rows than 64 bits count', dict(nframes=1 << 60)),
                ('rows overflow', 'more bytes than 2^62', dict(d_src=SRC, nframes=1 << 20, p__payload_nbytes=1 << 43)),
                ('row range', 'row_hi past the last row', dict(p__row_hi=4 * 768 + 8)),
            ] + SOURCE_RULES[:2] + [
                ('last bin', 'the last row past the last bin', dict(nbins=1)),
            ] + SOURCE_RULES[2:])
add('null parameter block', p=None)
add('nframes 0, null buffers', nframes=0, p__row_hi=0, d_buf=None, buf_nbytes=0)
add('rows and first_row past 64 bits', d_src=SRC, nframes=(1 << 21) - 1, p__bps=1, p__payload_nbytes=1 << 40,
    p__row_hi=((1 << 21) - 1) << 43, bin_rows=8, first_row=1 << 56, nbins=8)


def repack(**f):
    d = dict(bps=2, coder_in=0, coder_out=1, chunk_in=1, nslot_in=2, chunk_out=2, nslot_out=1, fill_code=0,
             payload_in=192, payload_out=64, src0=0, src_stride=192, row_lo=0, row_hi=8, first_row=0, reserved=0)
    d.update(f)
    return S('RepackParams', **d)


# 4 frame sets of 2 slots x 192 bytes (768 rows each) -> payloads of 64 bytes, 128 rows of 2 codes
RP = ['d_buf', 'buf_nbytes', 'd_src', 'nframes', 'p', 'd_out', 'out_nbytes', 'stream']
add = rules('bb_repack_frames', RP,
            dict(d_buf=BUF, buf_nbytes=8 * 192, d_src=None, nframes=4, p=repack(), d_out=OUT, out_nbytes=1 << 16, stream=None),
            [
                ('bps', '3 bits per sample', dict(p__bps=3)),
                ('fields', 'reserved set', dict(p__reserved=1)),
                ('fields', 'chunk_in 0', dict(p__chunk_in=0)),
                ('fields', 'nslot_in 0', dict(p__nslot_in=0)),
                ('fields', 'chunk_out 0', dict(p__chunk_out=0)),
                ('fields', 'nslot_out 0', dict(p__nslot_out=0)),
                ('code map', 'VDIF to INT', dict(p__coder_out=2)),
                ('code map', 'unknown coder', dict(p__coder_in=7)),
                ('pow2', 'chunk_in not a power of two', dict(p__chunk_in=3, p__chunk_out=6)),
                ('pow2', 'nslot_out not a power of two', dict(p__nslot_in=6, p__nslot_out=3)),
                ('samples', 'complete samples differ', dict(p__chunk_out=4)),
                ('slots', '64 slots in', dict(p__nslot_in=64, p__chunk_out=64)),
                ('slots', '64 slots out', dict(p__nslot_out=64, p__chunk_in=64)),
                ('row bits', 'rows of more than 256 bits', dict(p__chunk_in=128, p__nslot_out=8, p__chunk_out=32)),
                ('payload in', 'payload_in not whole dwords', dict(p__payload_in=190)),
                ('payload in', 'empty payload_in', dict(p__payload_in=0)),
                ('payload in', 'payload_in above 2^56', dict(p__payload_in=(1 << 56) + 4)),
                ('payload out', 'payload_out not whole dwords', dict(p__payload_out=62)),
                ('payload out', 'empty payload_out', dict(p__payload_out=0)),
                ('payload out', 'payload_out above 2^56', dict(p__payload_out=(1 << 56) + 4)),
                ('whole rows in', 'payload_in not whole rows', dict(p__payload_in=196, p__chunk_in=32, p__chunk_out=64)),
                ('whole rows out', 'payload_out not whole rows', dict(p__payload_out=68, p__chunk_in=16, p__chunk_out=32)),
                ('fill', 'negative fill_code', dict(p__fill_code=-1)),
                ('fill', 'fill_code 4', dict(p__fill_code=4)),
                ('row order', 'row_lo past row_hi', dict(p__row_lo=16)),
                ('output', 'null output', dict(d_out=None)),
                ('output', 'output not 16-byte aligned', dict(d_out=OUT + 8)),
                ('first_row', 'first_row above 2^56', dict(p__first_row=(1 << 56) + 8)),
                ('whole bytes', 'first_row not a whole byte', dict(p__first_row=2)),
                ('whole bytes', 'row_lo not a whole byte', dict(p__row_lo=2)),
                ('whole bytes', 'row_hi not a whole byte', dict(p__row_hi=10)),
                ('rows overflow', 'more rows than 64 bits count', dict(nframes=1 << 60)),
                ('rows overflow', 'more bytes than 2^58', dict(d_src=SRC, nframes=1 << 20, p__payload_in=1 << 39)),
                ('row range', 'row_hi past the last row', dict(p__row_hi=4 * 768 + 8)),
                ('empty', 'no rows', dict(p__row_lo=8)),
                ('empty', 'nframes 0', dict(nframes=0, p__row_hi=0)),
                ('output frames', 'more output bytes than 2^58', dict(p__first_row=1 << 56, p__chunk_in=16, p__chunk_out=32)),
                ('output range', 'output one byte short', dict(out_nbytes=3)),
                ('buffer', 'null buffer', dict(d_buf=None)),
                ('buffer', 'buffer not 4-byte aligned', dict(d_buf=BUF + 2)),
                ('stride', 'misaligned src0', dict(p__src0=2)),
                ('stride', 'negative src0', dict(p__src0=-4)),
                ('stride', 'misaligned src_stride', dict(p__src_stride=194)),
                ('stride', 'negative src_stride', dict(p__src_stride=-192)),
                ('source range', 'source range one byte past the end', dict(buf_nbytes=8 * 192 - 1)),
            ])
add('null parameter block', p=None)
add('nframes 0, null buffers', nframes=0, p__row_hi=0, d_buf=None, buf_nbytes=0)
add('second output frame one byte short', p__first_row=128, out_nbytes=67)


def requant(**f):
    d = dict(bps_in=2, bps_out=4, chunk=1, nslot=2, fill_code=0, reserved=0, payload_in=192, payload_out=64,
             src0=0, src_stride=192, row_lo=0, row_hi=8, first_row=0, map=[0, 5, 10, 15])
    d.update(f)
    return S('RequantParams', **d)


# 4 frame sets of 2 slots x 192 bytes (768 rows of one 2-bit code) -> payloads of 64 bytes, 128 rows of one 4-bit code
add = rules('bb_requant_frames', RP,
            dict(d_buf=BUF, buf_nbytes=8 * 192, d_src=None, nframes=4, p=requant(), d_out=OUT, out_nbytes=1 << 16, stream=None),
            [
                ('bps', '3 bits per sample in', dict(p__bps_in=3)),
                ('bps', '3 bits per sample out', dict(p__bps_out=3)),
                ('fields', 'reserved set', dict(p__reserved=1)),
                ('fields', 'chunk 0', dict(p__chunk=0)),
                ('fields', 'nslot 0', dict(p__nslot=0)),
                ('pow2', 'chunk not a power of two', dict(p__chunk=3)),
                ('pow2', 'nslot not a power of two', dict(p__nslot=3)),
                ('slots', '64 slots', dict(p__nslot=64)),
                ('row bits', 'rows of more than 256 bits', dict(p__chunk=128)),
                ('payload in', 'payload_in not whole dwords', dict(p__payload_in=190)),
                ('payload in', 'empty payload_in', dict(p__payload_in=0)),
                ('payload in', 'payload_in above 2^56', dict(p__payload_in=(1 << 56) + 4)),
                ('payload out', 'payload_out not whole dwords', dict(p__payload_out=62)),
                ('payload out', 'empty payload_out', dict(p__payload_out=0)),
                ('payload out', 'payload_out above 2^56', dict(p__payload_out=(1 << 56) + 4)),
                ('whole rows in', 'payload_in not whole rows', dict(p__payload_in=196, p__chunk=32)),
                ('whole rows out', 'payload_out not whole rows', dict(p__payload_out=68, p__chunk=16)),
                ('fill', 'negative fill_code', dict(p__fill_code=-1)),
                ('fill', 'fill_code 16', dict(p__fill_code=16)),
                ('map', 'map entry 16 for 4 bits', dict(p__map=[0, 5, 10, 16])),
                ('row order', 'row_lo past row_hi', dict(p__row_lo=16)),
                ('output', 'null output', dict(d_out=None)),
                ('output', 'output not 16-byte aligned', dict(d_out=OUT + 8)),
                ('first_row', 'first_row above 2^56', dict(p__first_row=(1 << 56) + 8)),
                ('whole bytes', 'first_row not a whole byte', dict(p__first_row=2)),
                ('whole bytes', 'row_lo not a whole byte', dict(p__row_lo=2)),
                ('whole bytes', 'row_hi not a whole byte', dict(p__row_hi=10)),
                ('whole bytes', 'whole bytes in, not out', dict(p__bps_in=4, p__bps_out=2, p__payload_in=64, p__payload_out=192,
                                                                 p__src_stride=64, p__map=[0, 1, 2, 3], p__row_hi=10)),
                ('rows overflow', 'more rows than 64 bits count', dict(nframes=1 << 60)),
                ('rows overflow', 'more bytes than 2^58', dict(d_src=SRC, nframes=1 << 20, p__payload_in=1 << 39)),
                ('row range', 'row_hi past the last row', dict(p__row_hi=4 * 768 + 8)),
                ('empty', 'no rows', dict(p__row_lo=8)),
                ('empty', 'nframes 0', dict(nframes=0, p__row_hi=0)),
                ('output frames', 'more output bytes than 2^58', dict(p__first_row=1 << 56, p__chunk=16)),
                ('output range', 'output one byte short', dict(out_nbytes=67)),
                ('buffer', 'null buffer', dict(d_buf=None)),
                ('buffer', 'buffer not 4-byte aligned', dict(d_buf=BUF + 2)),
                ('stride', 'misaligned src0', dict(p__src0=2)),
                ('stride', 'negative src0', dict(p__src0=-4)),
                ('stride', 'misaligned src_stride', dict(p__src_stride=194)),
                ('stride', 'negative src_stride', dict(p__src_stride=-192)),
                ('source range', 'source range one byte past the end', dict(buf_nbytes=8 * 192 - 1)),
            ])
add('null parameter block', p=None)
add('nframes 0, null buffers', nframes=0, p__row_hi=0, d_buf=None, buf_nbytes=0)
add('second output frame one byte short', p__first_row=128, out_nbytes=195)

# pairs whose single-fault changes contradict each other, restated so that both faults stand
PAIRED_BY_HAND = {
    'bb_count_states': [
        ('empty + row range', dict(p__row_lo=4 * 768 + 8, p__row_hi=4 * 768 + 8)),
        ('empty + row order (nframes 0)', dict(nframes=0, p__row_lo=8, p__row_hi=0)),
        ('empty + row range (nframes 0)', dict(nframes=0)),
    ],
    'bb_count_states_bins': [
        ('empty + row range', dict(p__row_lo=4 * 768 + 8, p__row_hi=4 * 768 + 8)),
        ('empty + row range (nframes 0)', dict(nframes=0)),
        ('empty + whole bytes', dict(p__row_lo=2, p__row_hi=2)),
        ('whole bytes + row range', dict(p__row_hi=4 * 768 + 2)),
        ('whole bytes + first_row', dict(first_row=(1 << 56) + 2)),
    ],
    'bb_repack_frames': [
        ('empty + row range', dict(p__row_lo=4 * 768 + 8, p__row_hi=4 * 768 + 8)),
        ('empty + row range (nframes 0)', dict(nframes=0)),
        ('empty + whole bytes', dict(p__row_lo=2, p__row_hi=2)),
        ('whole bytes + row range', dict(p__row_hi=4 * 768 + 2)),
        ('whole bytes + first_row', dict(p__first_row=(1 << 56) + 2)),
    ],
    'bb_requant_frames': [
        ('empty + row range', dict(p__row_lo=4 * 768 + 8, p__row_hi=4 * 768 + 8)),
        ('empty + row range (nframes 0)', dict(nframes=0)),
        ('empty + whole bytes', dict(p__row_lo=2, p__row_hi=2)),
        ('whole bytes + row range', dict(p__row_hi=4 * 768 + 2)),
        ('whole bytes + first_row', dict(p__first_row=(1 << 56) + 2)),
    ],
}


def pair_cases(code_of):
    """The double-fault calls of PAIRED, given the codes the single faults answered."""
    npairs = nskipped = 0
    for fn, names, base, table in PAIRED:
        add = entry(fn, names, base)
        first = {}
        for statement, label, changes in table:
            first.setdefault(statement, (label, changes))
        reps = list(first.items())
        for i, (sa, (la, ca)) in enumerate(reps):
            for sb, (lb, cb) in reps[i + 1:]:
                if code_of['{}:{}'.format(fn, la)] == code_of['{}:{}'.format(fn, lb)]:
                    continue
                if any(k in cb and cb[k] != v for k, v in ca.items()):
                    nskipped += 1
                    continue
                add('{} + {}'.format(la, lb), **dict(ca, **cb))
                npairs += 1
        for label, changes in PAIRED_BY_HAND[fn]:
            add(label, **changes)
    return npairs, nskipped


def main():
    from baseband_amd import _lib
    assert abi_replay.device_is_hidden(), "record this table on a machine without a device"

    def record(cases):
        for c in cases:
            c['code'] = abi_replay.call(c)
            assert c['code'] != _lib.BB_EIO, "{}: passes its argument checks (BB_EIO): not a case for this table".format(c['id'])
            assert c['code'] in (_lib.BB_OK, _lib.BB_EINVAL, _lib.BB_ERANGE, _lib.BB_ENOTSUP), c

    record(CASES)
    nsingle = len(CASES)
    print("{} pairs of statements, {} left out (contradicting changes)".format(*pair_cases({c['id']: c['code'] for c in CASES})))
    record(CASES[nsingle:])
    CASES.sort(key=lambda c: c['fn'] == 'bb_requant_frames')         # recorded later: its rows stand behind the others'
    ids = [c['id'] for c in CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    path = os.path.join(ROOT, 'tests', 'golden', 'abi_return_codes.json')
    with open(path, 'w') as f:
        f.write('{"cases": [\n' + ',\n'.join(json.dumps(c, sort_keys=True) for c in CASES) + '\n]}\n')
    print("{} calls -> {}".format(len(CASES), path))


if __name__ == '__main__':
    main()
