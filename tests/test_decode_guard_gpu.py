"""Every decode kernel writes its output, the whole of it, and nothing else.

The other decode tests let the wrapper allocate the output (torch.empty of exactly the
needed size) and look at nothing but that tensor.  Three faults pass them: a work item
that clips its tail wrongly and stores past the last frame (allocator slack, or another
tensor), a launch that skips a tile and finds the previous launch's correct answer in a
recycled block, and a kernel that needs more than the 16-byte alignment the ABI asks for.

Here every launch decodes into a view of a poisoned allocation (tests/guardkit.py: 1 MiB
of guard either side, refilled before every launch) whose base is 0, 16 or 4080 bytes past
a 4096-byte boundary (4 and 12 too where the ABI takes 4-byte alignment), and
`guardkit.verdict` compares, on the device, with expectations worked out in NumPy
(tests/launch_expect.py): no guard element touched, no poison left, every value right.

  1. the 202 decode / Mark 4 / tiled / copy cases of tests/golden/launch_notes.json;
  2. tails that table does not have: payloads of 41 and 43 tiles and ones that end inside
     a tile, a last frame-slot that is a hole / at an odd address / out of the buffer,
     3 and 5 thread slots, a chunk wider than a work item, grids of 1 and 3 workgroups,
     the striped work order at an odd item count -- float32, float16 / bfloat16, Mark 4, copies;
  3. the three window entries, against the four separate calls;
  4. one reader per format, `read(out=view)` from a sample offset inside a frame.

The table was recorded with the product library: the experiment build words its notes
differently (tests/test_launch_notes_gpu.py) and is skipped for the same reason."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import guardkit
import launch_expect as le
import launch_replay
import test_kernels_gpu as tk
from conftest import golden_path, load_expected

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get('BB_EXPERIMENTS', '') not in ('', '0'),
                                 reason="recorded with the product library (_lib.EXPERIMENTS is set)")]

with open(golden_path('launch_notes.json')) as _f:
    CASES = [c for c in json.load(_f)['cases'] if c['op'] in le.OPS]

DELTAS = (0, 16, 4080)              # bytes from a 4096-byte boundary to the output
DELTAS_4B = (4, 12)                 # ... for the entries that take 4-byte aligned outputs
TAIL_DELTA = 16                     # part 2: 16-byte aligned and no more


def _torch_dtype(out):
    import torch
    return {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[out]


def _kernel(note):
    return note.split('<')[0]


def guarded(want, dtype, launch, delta, kernel=None, what=None):
    """One launch into a fresh poisoned view `delta` bytes past a page boundary; `launch(view)` returns the
    tensor the wrapper says it wrote.  Asserts that it is the view, that the launch left `want` and touched
    nothing else, and (if given) which kernel ran.  -> the bb_last_kernel() note."""
    from baseband_amd import _lib
    whole, view = guardkit.poisoned(want.size, dtype, delta)
    res = launch(view)
    note = _lib.last_kernel()
    assert res.data_ptr() == view.data_ptr() and res.numel() == view.numel(), (what, delta, "a temporary stood in")
    v = guardkit.verdict(whole, view, want)
    assert guardkit.clean(v), (what, delta, note, guardkit.describe(v, want.size))
    if kernel is not None:
        assert note.startswith(kernel), (what, note, kernel)
    return note


class knobs:
    """`with knobs(BLOCKS=3):` -- set for the launches inside, back to the library's defaults after."""
    DEFAULTS = dict(launch_replay.KNOB_DEFAULTS, WORK_STRIPES=-1)

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        from baseband_amd import kernels, _lib
        for k, v in self.kv.items():
            kernels.tune(getattr(_lib, 'TUNE_' + k), v)

    def __exit__(self, *exc):
        from baseband_amd import kernels, _lib
        for k in self.kv:
            kernels.tune(getattr(_lib, 'TUNE_' + k), self.DEFAULTS[k])


# ---- 1. the recorded cases ----------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_recorded_case_into_a_guarded_output(case):
    a = case['args']
    want = le.expected(case)
    dtype = _torch_dtype(a.get('out', 'f32'))
    takes_4b = 'within' in a or bool(a.get('nout', 0))     # bb_decode_frames_select, bb_decode_mark4_select
    # (the case recorded with an output one float off the 16-byte grid keeps that float)
    extra = 4 * a.get('out_offset', 0)
    for delta in DELTAS + (DELTAS_4B if takes_4b else ()):
        note = guarded(want, dtype, lambda view: launch_replay.launch(case, out=view)[1], delta + extra, what=case['id'])
        if delta % 16 == 0:
            assert note == case['note'], delta
        else:
            # the float4 / scalar wording follows the alignment; and k_decode_pick stores float4 only, so off
            # the 16-byte grid its cases are k_decode_gather_select's (bb_decode_frames_select)
            recorded = _kernel(case['note'])
            assert _kernel(note) == ('k_decode_gather_select' if recorded == 'k_decode_pick' else recorded), delta
            assert ('scalar' in note) == bool((delta + extra) % 16), (delta, note)


# ---- 2. tails the table does not have -------------------------------------------------------------------
TILE_PAYLOADS = (10496, 11008)                  # 41 and 43 tiles of 256 bytes
INSIDE_PAYLOADS = (4, 8, 260, 8196)             # end inside a tile
PAYLOADS = TILE_PAYLOADS + INSIDE_PAYLOADS
PLACES = ('hole', 'odd', 'past', 'fixed')       # the last frame-slot; 'fixed': no index at all
NFRAMES = 5
STRIPED_ITEMS = 259                             # odd, 64 items in each of BB_TUNE_WORK_STRIPES = 2 -> 4 stripes, 3 left over
FILL = 7.25, -0.375


def _tail_input(seed, nfs, unit, place, align=4):
    """Random bytes holding `nfs` units of `unit` bytes at a stride that walks through the alignments, and the
    index whose LAST entry is a hole, at an odd byte address, or names a unit that ends outside the buffer."""
    rng = np.random.default_rng(seed)
    head = 32
    stride = unit + 36 + (-(unit + 36)) % align
    raw = rng.integers(0, 256, head + nfs * stride + 8, dtype=np.uint8)
    src = head + np.arange(nfs, dtype=np.int64) * stride
    if place == 'hole':
        src[-1] = -1
    elif place == 'odd':
        src[-1] += 1
    elif place == 'past':
        src[-1] = raw.size - unit + align
    return raw, head, stride, src


def _runs(payloads=PAYLOADS):
    """(payload, place, BB_TUNE_BLOCKS) of the tails: every placement on the default grid, the hole on grids of
    1 and 3 workgroups (they loop over the work items)."""
    for pn in payloads:
        for place in PLACES:
            yield pn, place, None
        for blocks in (1, 3):
            yield pn, 'hole', blocks


def _decode_tail(coder, bps, pn, nframes, nslot, chunk, place, out, kernel, blocks=None, stripes=None, staged=False):
    import torch
    from baseband_amd import kernels
    cplx = chunk % 2 == 0
    raw, head, stride, src = _tail_input(pn * 31 + nslot, nframes * nslot, pn, place)
    want = le.as_out_type(le.decode_values(raw, src, nframes, nslot, chunk, pn, tk.CODERS[coder], bps, cplx, fill=FILL), out)
    dbuf = kernels.to_device_bytes(raw)
    kw = dict(chunk=chunk, nslot=nslot, complex_data=cplx, fill_value=complex(*FILL) if cplx else FILL[0],
              out_dtype=_torch_dtype(out))
    if place == 'fixed':
        kw.update(src0=head, src_stride=stride)
    else:
        kw['src'] = torch.from_numpy(src).cuda()
    what = (coder, bps, pn, nframes, nslot, chunk, place, out, blocks, stripes)
    with knobs(BLOCKS=blocks, WORK_STRIPES=stripes, VDIF8_LDS_GIB=0 if staged else None):
        note = guarded(want.reshape(-1), _torch_dtype(out),
                       lambda view: kernels.decode_frames(dbuf, nframes, pn, tk.CODERS[coder], bps, out=view, **kw),
                       TAIL_DELTA, kernel, what)
    if blocks:
        assert 1 <= int(re.search(r' grid (\d+)', note).group(1)) <= blocks, note


# (coder, bits, VDIF 8-bit through the staged kernel?) -> the kernel of a contiguous float32 output
FLAT = [('vdif', 1, False, 'k_decode_flat_lut<1,'), ('mark5b', 1, False, 'k_decode_flat_lut<1,'),
        ('vdif', 2, False, 'k_decode_flat_lds<2,'), ('mark5b', 2, False, 'k_decode_flat_lds<2,'),
        ('vdif', 4, False, 'k_decode_flat_lds<4,'), ('int', 4, False, 'k_decode_flat_lds<4,'),
        ('vdif', 8, False, 'k_decode_flat<8,LDS,0,'), ('vdif', 8, True, 'k_decode_flat_lds<8,LDS,'),
        ('int', 8, False, 'k_decode_flat_lds<8,INT8,')]


@pytest.mark.parametrize('coder,bps,staged,kernel', FLAT, ids=['{}{}{}'.format(c, b, '-staged' if s else '') for c, b, s, _ in FLAT])
def test_flat_tails(coder, bps, staged, kernel):
    for pn, place, blocks in _runs():
        _decode_tail(coder, bps, pn, NFRAMES, 1, 1, place, 'f32', kernel, blocks, staged=staged)
    _decode_tail(coder, bps, 260, STRIPED_ITEMS, 1, 1, 'hole', 'f32', kernel, stripes=2, staged=staged)


def _interleave_kernel(nslot, chunk, place):
    """bb_decode_frames' choice for a float32 thread interleave (csrc/bbdecode.hip)."""
    rows4 = chunk % 4 == 0
    if place != 'fixed' and (not rows4 or nslot <= 4 or chunk < 32):
        return 'k_decode_gather<'
    return 'k_decode_rows_pipe<' if rows4 else 'k_decode_flat<'


# thread slots x chunk; the last: a chunk (4096 floats) wider than a work item, payload 8192 only
SHAPES = [(3, 2), (3, 4), (3, 16), (5, 2), (5, 4), (5, 16), (5, 32), (8, 32), (2, 4096)]
WIDTHS = [('vdif', 1), ('vdif', 2), ('vdif', 4), ('vdif', 8), ('int', 8)]      # the <BPS, LV> instantiations


def _fits(pn, bps, chunk):
    return (pn * 8 // bps) % chunk == 0


@pytest.mark.parametrize('nslot,chunk', SHAPES, ids=['{}x{}'.format(*s) for s in SHAPES])
@pytest.mark.parametrize('coder,bps', WIDTHS, ids=['{}{}'.format(*w) for w in WIDTHS])
def test_interleave_tails(coder, bps, nslot, chunk):
    ran = 0
    for pn, place, blocks in _runs((8192,) if chunk == 4096 else PAYLOADS):
        if _fits(pn, bps, chunk):
            _decode_tail(coder, bps, pn, NFRAMES, nslot, chunk, place, 'f32', _interleave_kernel(nslot, chunk, place), blocks)
            ran += 1
    assert ran >= 6
    # the striped order: one work item per frame set (a payload of two tiles; 8 slots: one group of waves)
    if (nslot, chunk) in ((3, 4), (8, 32)):
        pn = 288
        assert _fits(pn, bps, chunk)
        _decode_tail(coder, bps, pn, STRIPED_ITEMS, nslot, chunk, 'hole', 'f32', _interleave_kernel(nslot, chunk, 'hole'),
                     stripes=2)


@pytest.mark.parametrize('out', ['f16', 'bf16'])
@pytest.mark.parametrize('coder,bps', WIDTHS, ids=['{}{}'.format(*w) for w in WIDTHS])
def test_half_tails(coder, bps, out):
    flat, rows = 'k_decode_half_flat<{},'.format(bps), 'k_decode_half_rows<{}>'.format(bps)
    for pn, place, blocks in _runs():
        _decode_tail(coder, bps, pn, NFRAMES, 1, 1, place, out, flat, blocks)
    _decode_tail(coder, bps, 260, STRIPED_ITEMS, 1, 1, 'hole', out, flat, stripes=2)
    for nslot, chunk in ((3, 2), (5, 4), (5, 16), (2, 4096)):
        for pn, place, blocks in _runs((8192,) if chunk == 4096 else PAYLOADS):
            if _fits(pn, bps, chunk):
                _decode_tail(coder, bps, pn, NFRAMES, nslot, chunk, place, out, rows, blocks)
    # (payload 8: one work item of 8 bytes per slot and frame set)
    _decode_tail(coder, bps, 8, STRIPED_ITEMS, 3, 2, 'hole', out, rows, stripes=2)


SELECTS = [(3, 16, [1, 4, 6]), (5, 16, [5]), (8, 16, [5]), (5, 8, [0, 2, 3, 7])]


@pytest.mark.parametrize('nslot,chunk,within', SELECTS, ids=['{}x{} keep {}'.format(s, c, len(w)) for s, c, w in SELECTS])
def test_select_tails(nslot, chunk, within):
    """bb_decode_frames_select (k_decode_gather_select, k_decode_pick): the same tails, outputs on and off the
    16-byte grid."""
    import torch
    from baseband_amd import kernels
    wdev = torch.tensor(within, dtype=torch.int32, device='cuda')
    for coder, bps in (('vdif', 2), ('int', 8)):
        for pn, place, blocks in _runs():
            if place == 'fixed' or not _fits(pn, bps, chunk):
                continue
            raw, head, stride, src = _tail_input(pn + nslot, NFRAMES * nslot, pn, place)
            want = le.decode_values(raw, src, NFRAMES, nslot, chunk, pn, tk.CODERS[coder], bps, False, fill=FILL, within=within)
            dbuf, dsrc = kernels.to_device_bytes(raw), torch.from_numpy(src).cuda()
            for delta in (TAIL_DELTA, 4):
                with knobs(BLOCKS=blocks):
                    note = guarded(want.reshape(-1), torch.float32,
                                   lambda view: kernels.decode_frames(dbuf, NFRAMES, pn, tk.CODERS[coder], bps, chunk=chunk,
                                                                      nslot=nslot, src=dsrc, fill_value=FILL[0], within=wdev,
                                                                      out=view),
                                   delta, what=(coder, bps, nslot, chunk, within, pn, place, blocks))
                assert _kernel(note) in ('k_decode_gather_select', 'k_decode_pick'), note
                if delta % 16:
                    assert 'scalar' in note, note


M4_WORDS = (41 * 64, 43 * 64, 4, 8, 260, 8196)      # 41 and 43 tiles of 64 words; units that end inside a tile


@pytest.mark.parametrize('select', [False, True], ids=['all', 'select'])
@pytest.mark.parametrize('widen', [1, 0], ids=['super-words', 'native'])
@pytest.mark.parametrize('ntrack', [16, 32, 64])
def test_mark4_tails(ntrack, widen, select):
    import torch
    from baseband_amd import kernels
    rng = np.random.default_rng(ntrack + widen)
    perm = rng.permutation(ntrack)
    sign, mag = [int(x) for x in perm[:ntrack // 2]], [int(x) for x in perm[ntrack // 2:]]
    if select:
        sign, mag = sign[:3], mag[:3]
    wbytes = ntrack // 8
    seen = set()
    for nwords, place, blocks in _runs(M4_WORDS):
        for fill_words in (0, 7, 160):
            if fill_words > nwords or (blocks and fill_words == 7):
                continue
            nframes = NFRAMES
            raw, head, stride, src = _tail_input(nwords + fill_words, nframes, nwords * wbytes, place, align=8)
            want = le.mark4_values(raw, src, nframes, ntrack, nwords, sign, mag, fill_words, fill=FILL[0])
            dbuf = kernels.to_device_bytes(raw)
            kw = dict(src0=head, src_stride=stride) if place == 'fixed' else dict(src=torch.from_numpy(src).cuda())
            r = 64 // ntrack
            wide = bool(widen) and r > 1 and nwords % r == 0 and fill_words % r == 0 and len(sign) * r <= 32
            kernel = 'k_decode_mark4{}<{},'.format('_select' if select else '', 64 if wide else ntrack)
            with knobs(BLOCKS=blocks, M4_WIDEN=widen):
                note = guarded(want.reshape(-1), torch.float32,
                               lambda view: kernels.decode_mark4(dbuf, nframes, ntrack, nwords, sign, mag, fill_words=fill_words,
                                                                 fill_value=FILL[0], select=select, out=view, **kw),
                               TAIL_DELTA, kernel, (ntrack, widen, select, nwords, place, blocks, fill_words))
            assert ('super-words' in note) == wide, note
            seen.add(wide)
            if select and not blocks and place == 'odd':          # bb_decode_mark4_select takes 4-byte aligned outputs
                with knobs(M4_WIDEN=widen):
                    note = guarded(want.reshape(-1), torch.float32,
                                   lambda view: kernels.decode_mark4(dbuf, nframes, ntrack, nwords, sign, mag,
                                                                     fill_words=fill_words, fill_value=FILL[0], select=True,
                                                                     out=view, **kw),
                                   4, kernel, (ntrack, widen, 'select at 4', nwords, fill_words))
                assert 'scalar' in note, note
    assert seen == ({True, False} if (widen and ntrack < 64) else {False})      # (7 fill words are never widened)
    # the striped work order: one item per unit
    nwords = 260
    raw, head, stride, src = _tail_input(5, STRIPED_ITEMS, nwords * wbytes, 'hole', align=8)
    want = le.mark4_values(raw, src, STRIPED_ITEMS, ntrack, nwords, sign, mag, 7, fill=FILL[0])
    dbuf, dsrc = kernels.to_device_bytes(raw), torch.from_numpy(src).cuda()
    with knobs(WORK_STRIPES=2, M4_WIDEN=widen):
        guarded(want.reshape(-1), torch.float32,
                lambda view: kernels.decode_mark4(dbuf, STRIPED_ITEMS, ntrack, nwords, sign, mag, fill_words=7, src=dsrc,
                                                  fill_value=FILL[0], select=select, out=view), TAIL_DELTA, what='striped')


# bytes per run, offset of the first, stride -> the 16-byte or the 4-byte form; 16400 and 16388: two work items per run
COPIES = [(n, 64, n + 48, '16B') for n in TILE_PAYLOADS + (16, 16400)] + \
         [(n, 12, n + 36, '4B') for n in INSIDE_PAYLOADS + (16388,)] + [(10496, 12, 10496 + 36, '4B')]


def test_copy_tails():
    import torch
    from baseband_amd import kernels
    rng = np.random.default_rng(40)
    for n, src0, stride, form in COPIES:
        for nframes, blocks, stripes in ((NFRAMES, None, None), (NFRAMES, 1, None), (NFRAMES, 3, None),
                                         (STRIPED_ITEMS, None, 2)):
            if stripes and n > 16384:
                continue                                    # (two items per run: an even item count)
            raw = rng.integers(0, 256, src0 + nframes * stride, dtype=np.uint8)
            raw.view(np.uint32)[raw.view(np.uint32) == guardkit.POISON] = 0         # (never drawn; and said so)
            want = le.copy_values(raw, nframes, n, src0, stride)
            dbuf = kernels.to_device_bytes(raw)
            with knobs(BLOCKS=blocks, WORK_STRIPES=stripes):
                guarded(want, torch.float32,
                        lambda view: kernels.copy_frames(dbuf, nframes, n, src0=src0, src_stride=stride, out=view),
                        TAIL_DELTA, 'k_copy_frames<nt,{},'.format(form), (n, src0, stride, nframes, blocks, stripes))


# ---- 3. the window entries ---------------------------------------------------------------------------------

def _window_into_views(want, run, what):
    """`run(out)` decodes a window into `out`: a view of a poisoned allocation at element offsets 0, 4 and 1 (the
    last off the 16-byte grid: a temporary inside, copied into place).  The view holds what the four separate
    calls gave, and every other element of the allocation is still poison."""
    import torch
    bits = want.reshape(-1).cpu().numpy()
    for off in (0, 4, 1):
        whole, view = guardkit.poisoned(bits.size, torch.float32, 4 * off)
        run(view)
        v = guardkit.verdict(whole, view, bits)
        assert guardkit.clean(v), (what, off, guardkit.describe(v, bits.size))


def test_vdif_window_into_guarded_views():
    import torch
    from baseband_amd import kernels, synth, _lib
    image, h0 = synth.random_vdif(3, 9, nthread=4, nchan=2, bps=2, payload_nbytes=64, frame_rate=4,
                                  thread_order=[2, 0, 3, 1], invalid=[(1, 2), (5, 0)])
    image = image.copy()
    fn = h0.frame_nbytes
    image[7 * fn + 8] ^= 0xff            # corrupt frame_length of file frame 7
    pattern, mask = h0.invariant_pattern()
    dbuf = kernels.to_device_bytes(image)
    for threads, within in (([0, 1, 2, 3], None), ([3, 0], None), ([0, 1, 2, 3], [1]), ([2], [0, 1])):
        nslot = len(threads)
        slot = kernels.thread_slot_map(threads, dbuf.device)
        wdev = None if within is None else torch.tensor(within, dtype=torch.int32, device='cuda')
        for first, nsets in ((0, 9), (2, 5), (8, 1)):
            sub = dbuf[first * 4 * fn:]
            nframes = nsets * 4
            recs = kernels.vdif_scan(sub, nframes, fn, 32, pattern, mask, h0['seconds'], h0['frame_nr'] + first, 4)
            src = kernels.build_index(recs, nsets, nslot, slot)
            want = kernels.decode_frames(sub, nsets, 64, _lib.CODER_VDIF, 2, chunk=2, nslot=nslot, src=src,
                                         fill_value=-3.5, within=wdev)
            w = kernels.VDIFWindow(fn, 32, pattern, mask, h0['seconds'], 4, 64, _lib.CODER_VDIF, 2, 2, nslot, False, -3.5)
            _window_into_views(want, lambda out: w.run(sub, h0['frame_nr'] + first, nframes, slot, nsets, wdev, out, 4,
                                                       nframes, None, None), (threads, within, first))


def test_mark5b_window_into_guarded_views():
    import torch
    import bb_index_np as ix
    from baseband_amd import kernels, _lib
    rng = np.random.default_rng(51)
    F, n = ix.M5B_FRAME, 5
    buf = rng.integers(0, 256, (n + 1) * F, dtype=np.uint8)
    for k in range(n + 1):
        fnr = {3: 45}.get(k, k)                                     # one frame out of place: a hole in the index
        buf[k * F:k * F + 16] = ix.words_to_bytes(ix.mark5b_header_words(frame_nr=fnr, jday=321, seconds=777))
    buf[1 * F + 16:2 * F] = np.tile(ix.words_to_bytes([ix.M5B_FILL]), 2500)      # invalid
    dbuf = kernels.to_device_bytes(buf)
    ref = 321 * 86400 + 777
    recs = kernels.mark5b_scan(dbuf, n + 1, ref, 0, 6400)
    src = kernels.build_index(recs, n)
    assert int((src < 0).sum()) >= 1
    for nchan, within in ((4, None), (8, [1, 6])):
        wdev = None if within is None else torch.tensor(within, dtype=torch.int32, device='cuda')
        want = kernels.decode_frames(dbuf, n, 10000, _lib.CODER_MARK5B, 2, chunk=nchan, nslot=1, src=src, fill_value=-3.5,
                                     within=wdev)
        win = kernels.Mark5BWindow(ref, 6400, 2, nchan, -3.5)
        _window_into_views(want, lambda out: win.run(dbuf, 0, n + 1, n, wdev, out, n, None, None), (nchan, within))


@pytest.mark.parametrize('select', [False, True], ids=['all', 'select'])
def test_mark4_window_into_guarded_views(select):
    from baseband_amd import kernels, synth
    ntrack, n = 32, 3
    image, h0 = synth.random_mark4(17, n + 1, ntrack=ntrack, fanout=4, frame_rate=400, invalid=[1])
    dbuf = kernels.to_device_bytes(image)
    perm = np.random.default_rng(4).permutation(ntrack)
    sign, mag = [int(x) for x in perm[:ntrack // 2]], [int(x) for x in perm[ntrack // 2:]]
    if select:
        sign, mag = kernels.mark4_select_maps(sign, mag, 4, [2, 0])
    ref_qms, frame_qms = h0.time_quarter_ms(), 10
    for first in (0, 1):
        sub = dbuf[first * h0.frame_nbytes:]
        recs = kernels.mark4_scan(sub, n + 1 - first, ntrack, h0.year, ref_qms + first * frame_qms, frame_qms)
        src = kernels.build_index(recs, n - first)
        want = kernels.decode_mark4(sub, n - first, ntrack, 20000, sign, mag, fill_words=160, src=src, fill_value=-3.5,
                                    select=select)
        win = kernels.Mark4Window(ntrack, h0.year, ref_qms, frame_qms, 20000, sign, mag, select, 160, -3.5)
        _window_into_views(want, lambda out: win.run(sub, first, n + 1 - first, n - first, out, n - first, None, None),
                           (select, first))


# ---- 4. readers ----------------------------------------------------------------------------------------------

def _read_into_view(fh, start, count, want, what):
    """`fh.read(out=view)` from sample `start`, `view` inside a poisoned allocation at a 16-byte-only base."""
    import torch
    want = np.ascontiguousarray(want)
    cplx = np.iscomplexobj(want)
    bits = want.view(np.float32).reshape(-1)
    whole, view = guardkit.poisoned(bits.size, torch.float32, TAIL_DELTA)
    out = torch.view_as_complex(view.view(-1, 2)) if cplx else view
    out = out.view((count,) + tuple(want.shape[1:]))
    assert out.data_ptr() == view.data_ptr() and out.data_ptr() % 4096 == 16
    fh.seek(start)
    assert fh.read(out=out) is out and fh.tell() == start + count
    v = guardkit.verdict(whole, view, bits)
    assert guardkit.clean(v), (what, guardkit.describe(v, bits.size))
    return view


def test_vdif_reader_into_a_guarded_view():
    from baseband_amd import vdif
    exp = load_expected('sample_vdif').reshape(40000, 8)             # 8 threads, 20000 samples per frame
    with vdif.open(golden_path('samples/sample.vdif'), 'rs') as fh:
        _read_into_view(fh, 1234, 30001, exp[1234:31235], 'vdif')


def test_mark5b_reader_into_a_guarded_view():
    from baseband_amd import mark5b
    exp = load_expected('sample_m5b')                                # 5000 samples per frame
    with mark5b.open(golden_path('samples/sample.m5b'), 'rs', sample_rate=32e6, kday=56000, nchan=8, bps=2) as fh:
        _read_into_view(fh, 1234, 12001, exp[1234:13235], 'mark5b')


def test_mark4_reader_into_a_guarded_view():
    from baseband_amd import mark4
    exp = load_expected('sample_m4')                                 # 80000 samples per frame
    with mark4.open(golden_path('samples/sample.m4'), 'rs', ntrack=64, decade=2010) as fh:
        _read_into_view(fh, 1234, 100001, exp[1234:101235], 'mark4')


def test_guppi_reader_into_a_guarded_view(manifest):
    """With overlap: a read that starts inside a block follows the reference's loop, whose answer the manifest
    records by digest ('reads'); the values compared element by element are those of the plain read, which has
    that digest."""
    from baseband_amd import guppi
    start, count, digest = manifest['sample_puppi']['reads'][3]
    assert (start, count) == (1000, 1000)                            # 960 samples per block, 64 of them overlap
    with guppi.open(golden_path('samples/sample_puppi.raw'), 'rs') as fh:
        fh.seek(start)
        plain = fh.read(count).cpu().numpy()
        assert hashlib.sha256(plain.tobytes()).hexdigest() == digest
        view = _read_into_view(fh, start, count, plain, 'guppi')
    assert hashlib.sha256(view.cpu().numpy().tobytes()).hexdigest() == digest


def test_dada_reader_into_a_guarded_view(manifest):
    from baseband_amd import dada
    exp = load_expected('sample_dada')                               # one frame of 16000 samples
    start, count, digest = manifest['sample_dada']['reads'][4]
    assert (start, count) == (8001, 300)
    with dada.open(golden_path('samples/sample.dada'), 'rs') as fh:
        want = exp[start:start + count].reshape((count,) + tuple(fh.sample_shape))
        view = _read_into_view(fh, start, count, want, 'dada')
    assert hashlib.sha256(view.cpu().numpy().tobytes()).hexdigest() == digest
