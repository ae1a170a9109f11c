"""Every kernel family where its offsets need more than 31 or 32 bits.

The kernels keep frame, row and buffer offsets in wave-uniform 64-bit values and everything
inside a work item in 32 bits; the two meet at casts, magic-number divisions and clamps.
Here each family runs with source offsets, output offsets, offsets inside one payload and
row numbers either side of 2^31 and 2^32, on inputs that cost little to make
(tests/seamkit.py; tests/test_seamkit.py plants the faults these forms are there to find):

  * sparse sources     units at the places of `seamkit.places` in a buffer of 2^32 + 2^26
                       otherwise unwritten bytes, through an index;
  * a fixed stride     of 2^22 + 64 bytes, 1032 frame-slots from 8 MiB to past 2^32;
  * dense outputs      of 2^32 + 2^22 elements whose index is -1 but for the frame sets
                       around byte 2^31 .. 2^34 and element 2^31, 2^32 of the output;
  * periodic data      for what takes no index, and for single payloads past the seams.

One input buffer and one poisoned output allocation serve the whole module (the encoders'
float32 input and the buffer past 2^33 live for their own test only); the output is
poisoned again before every launch, every case names the kernel that ran (the packed-byte
entries and the scans leave no bb_last_kernel note: there the entry called is the kernel's),
and every comparison is exact.  The case lists are fixed here and every test counts what it
ran; tests/test_seamkit.py checks them, the fill values and the planted frames on the CPU."""
import numpy as np
import pytest

import bb_oracle_np as orc
import guardkit
import launch_expect as le
import seamkit as sk
import test_kernels_gpu as tk

pytestmark = pytest.mark.gpu

FILL = 7.25                         # no level of any coder, no int8 value (tests/test_seamkit.py)
M4_FILL = -6.5
CODER_WIDTHS = [('vdif', 1), ('vdif', 2), ('vdif', 4), ('vdif', 8), ('mark5b', 1), ('mark5b', 2), ('int', 4), ('int', 8)]

PN = 10496                          # payload of the sparse and dense decodes: 41 tiles, so no frame boundary on a seam
PN_STRIDE = 2304                    # ... at the fixed stride: 9 tiles
STRIDE_UNIT = 8192                  # random bytes at every stride; each family takes what it needs from their start
STRIDE_SRC0 = (1 << 23) + 64
STRIDE_N = 1032                     # frame-slots: 8 x 129 = 3 x 344

# (coder, bits, VDIF 8-bit through the staged kernel?) -> kernel of a contiguous float32 output
FLAT = [('vdif', 1, False, 'k_decode_flat_lut<1,'), ('vdif', 2, False, 'k_decode_flat_lds<2,'),
        ('vdif', 4, False, 'k_decode_flat_lds<4,'), ('vdif', 8, False, 'k_decode_flat<8,LDS,0,'),
        ('vdif', 8, True, 'k_decode_flat_lds<8,LDS,'), ('int', 8, False, 'k_decode_flat_lds<8,INT8,')]
WIDTHS = [('vdif', 1), ('vdif', 2), ('vdif', 4), ('vdif', 8), ('int', 8)]
SHAPES = [(3, 4), (8, 32)]          # thread slots x chunk: the gather (rows kernel without an index), the rows kernel
SELECTS = [(3, 16, (1, 4, 6), 'k_decode_gather_select<'), (8, 16, (5,), 'k_decode_pick<')]
HALF = [(out, coder, bps) for out in ('f16', 'bf16') for coder, bps in WIDTHS]
HALF_SHAPE = (3, 4)
# the family that also gets a buffer past 2^33: (coder, bits, slots, chunk, output type, kernel)
BEYOND = [('vdif', 2, 1, 1, 'f32', 'k_decode_flat_lds<2,'), ('vdif', 2, 3, 4, 'f32', 'k_decode_gather<'),
          ('vdif', 2, 8, 32, 'f32', 'k_decode_rows_pipe<'), ('int', 8, 1, 1, 'f16', 'k_decode_half_flat<8,'),
          ('vdif', 4, 3, 4, 'bf16', 'k_decode_half_rows<4>')]

# Mark 4: (tracks, BB_TUNE_M4_WIDEN, fill_words, select)
MARK4 = [(nt, w, fw, False) for nt in (16, 32, 64) for w in (1, 0) for fw in (0, 160)] + \
        [(32, 1, 160, True), (32, 0, 0, True)]
M4_WORDS = 2624                     # 41 tiles of 64 words
M4_WORDS_STRIDE = 328

COPY_PERIOD = 8191                  # an odd prime number of 16-byte (4-byte) rows
COPIES = [('16B', 16), ('4B', 4)]
BIG_PAYLOADS = [('int', 8, (1 << 32) + (1 << 20), 'f32', 'k_decode_flat_lds<8,INT8,'),
                ('int', 8, (1 << 32) + (1 << 20), 'f16', 'k_decode_half_flat<8,'),
                ('int', 4, (1 << 31) + (1 << 20), 'f32', 'k_decode_flat_lds<4,')]
BIG_PERIOD = 8191 * 4               # bytes: an odd prime number of dwords

# int8 transposes: (layout, polarisations, channels, times) -- at the fixed stride (k_decode_i8_xpose), with a channel
# list and the second of two polarisations there (k_decode_i8_xpose, k_decode_i8_tf_pick for time-first blocks), and
# through an index (k_decode_i8_tiled, k_decode_i8_stage)
TILED_FILL = FILL, FILL
XPOSE = [(0, 2, 8, 128), (1, 1, 8, 256), (2, 2, 8, 128)]
XPOSE_PICK = [(0, 64, 'k_decode_i8_xpose<0,'), (1, 256, 'k_decode_i8_xpose<1,'), (2, 64, 'k_decode_i8_tf_pick<')]
PICK_CHANNELS, PICK_STORED = (5, 0, 3, 6), 8
TILED = [(0, 2, 16, 82, 'k_decode_i8_tiled<0,'), (1, 2, 6, 256, 'k_decode_i8_stage<1,'), (2, 2, 16, 82, 'k_decode_i8_stage<2,')]

# encoders: more than 2^32 input elements of periodic float32
ENCODE_ELEMS = (1 << 32) + (1 << 22)
ENCODE_PERIOD = 8191 * 16           # elements: an odd prime number of 16-sample rows (whole output dwords at 2 bits)
ENCODES = [('vdif', 2), ('vdif', 4), ('vdif', 8)]
ENCODES_M4 = [64, 16]

CASE_COUNTS = dict(FLAT=6, WIDTHS=5, SHAPES=2, SELECTS=2, HALF=10, MARK4=14, COPIES=2, BIG_PAYLOADS=3,
                   XPOSE=3, XPOSE_PICK=3, TILED=3, ENCODES=3, ENCODES_M4=2, BEYOND=5)


def dense_shapes():
    """(coder, bits, thread slots, chunk, payload) of every dense-output decode: what tests/test_seamkit.py
    checks the frame sizes of."""
    for coder, bps, _, _ in FLAT:
        yield coder, bps, 1, 1, PN
    for coder, bps in WIDTHS:
        for nslot, chunk in SHAPES + [HALF_SHAPE]:
            yield coder, bps, nslot, chunk, PN


# ---- the module's buffers ----------------------------------------------------------------------------

def _need(nbytes):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("{:.1f} GiB of device memory free, {:.1f} needed".format(free / 2 ** 30, nbytes / 2 ** 30))


class _Buffers:
    strided = None                  # the units at the fixed stride, while the input buffer holds them


@pytest.fixture(scope='module')
def inbuf():
    import torch
    _need(sk.SIZE + (1 << 30))
    buf = torch.empty(sk.SIZE, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    _Buffers.strided = None
    yield buf
    _Buffers.strided = None


@pytest.fixture(scope='module')
def outalloc():
    import torch
    _need(4 * sk.OUT_ELEMS + (4 << 30))
    torch.cuda.reset_peak_memory_stats()
    whole = sk.allocation(4 * sk.OUT_ELEMS, 'cuda')
    yield whole
    print("\ntest_seams_gpu: peak device memory {:.2f} GiB".format(torch.cuda.max_memory_allocated() / 2 ** 30))


def _tdtype(out):
    import torch
    return {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[out]


def _item(out):
    return 4 if out == 'f32' else 2


def _fill_bits(value, out):
    return int(le.as_out_type(np.array([value], np.float32), out).view(np.uint32 if out == 'f32' else np.uint16)[0])


def _view(outalloc, nelem, out):
    """Poison the allocation again; -> (first element, view of `nelem` elements of output type `out`)."""
    guardkit.refill(outalloc)
    return sk.view_of(outalloc, nelem, _tdtype(out), _item(out))


def _strided(inbuf):
    if _Buffers.strided is None:
        _Buffers.strided = sk.Strided(inbuf, STRIDE_SRC0, sk.STRIDE, STRIDE_N, STRIDE_UNIT, np.random.default_rng(77))
        s = _Buffers.strided
        assert s.index()[-1] > sk.HIGH and len(s.crossing(sk.LOW)) == 3 and len(s.crossing(sk.HIGH)) == 3
        s.small, s.cidx = s.compact()
    return _Buffers.strided


def _sparse(inbuf, unit, seed, align=4):
    """Random units at the seam places; they stay clear of the units at the fixed stride."""
    at = sk.places(unit, sk.SIZE, align=align)
    if _Buffers.strided is not None:
        lo = _Buffers.strided.index()
        for p in at:
            assert not ((lo < p + unit) & (p < lo + STRIDE_UNIT)).any(), p
    sp = sk.Sparse(inbuf, unit, at, np.random.default_rng(seed))
    sp.small, sp.cidx = sp.compact()
    return sp


def _small(outalloc, out, want, launch, kernel, what):
    """One launch into a small view of the poisoned allocation, judged by guardkit."""
    from baseband_amd import _lib
    want = np.ascontiguousarray(want).reshape(-1)
    assert not guardkit.contains_poison(want), what
    lo, view = _view(outalloc, want.size, out)
    res = launch(view)
    note = _lib.last_kernel()
    assert res.data_ptr() == view.data_ptr(), (what, "a temporary stood in")
    v = guardkit.verdict(outalloc[:(2 * guardkit.GUARD + want.nbytes + 3) // 4], view, want)
    assert guardkit.clean(v), (what, note, guardkit.describe(v, want.size))
    assert note.startswith(kernel), (what, note, kernel)
    return note


def _dense(outalloc, out, nelem, fill_value, live, launch, kernel, what):
    """One launch into a view of `nelem` elements, all fill but the `live` ranges; judged on the device."""
    from baseband_amd import _lib
    for _, e in live:
        assert not guardkit.contains_poison(e), what
    lo, view = _view(outalloc, nelem, out)
    res = launch(view)
    note = _lib.last_kernel()
    assert res.data_ptr() == view.data_ptr(), (what, "a temporary stood in")
    v = sk.dense_verdict(outalloc, lo, nelem, _item(out), _fill_bits(fill_value, out), live)
    assert guardkit.clean(v), (what, note, guardkit.describe(v, nelem))
    assert note.startswith(kernel), (what, note, kernel)
    return note


@pytest.mark.parametrize('out', ['f32', 'f16'])
def test_device_verdicts_see_faults_past_the_seams(outalloc, out):
    """The verdicts themselves at full size, on the device: an output written with torch, then one wrong value, one
    element never stored and one store behind the view, all past element 2^32."""
    import torch
    nelem, item = sk.OUT_ELEMS - 12, _item(out)
    lo, view = _view(outalloc, nelem, out)
    view.fill_(FILL)
    first = np.arange(1, 45, dtype=np.float32)
    live = [((1 << 32) - 20, le.as_out_type(first, out))]
    view[(1 << 32) - 20:(1 << 32) + 24] = torch.from_numpy(first).cuda().to(_tdtype(out))
    fill = _fill_bits(FILL, out)
    assert sk.dense_verdict(outalloc, lo, nelem, item, fill, live) == ([], 0, 0)
    view[(1 << 32) + 3] = 99.
    view[(1 << 32) + 1000] = 98.
    ints = sk._ints(outalloc, item)
    ints[lo + (1 << 32) + 2000] = sk._signed(guardkit.POISON >> (16 * ((lo + 2000) % 2)) if item == 2 else guardkit.POISON, item)
    ints[lo + nelem + 2] = 0
    assert sk.dense_verdict(outalloc, lo, nelem, item, fill, live) == ([nelem + 2], 1, 2)
    # ... and the periodic one: 7 elements over and over, one of them wrong past 2^32
    lo, view = _view(outalloc, nelem, out)
    seven = le.as_out_type(np.arange(7, dtype=np.float32) - 3, out)
    sk._ints(outalloc, item)[lo:lo + nelem // 7 * 7].view(-1, 7)[:] = torch.from_numpy(sk._bits(seven, item)).cuda()
    sk._ints(outalloc, item)[lo + nelem // 7 * 7:lo + nelem] = torch.from_numpy(sk._bits(seven, item)[:nelem % 7]).cuda()
    assert sk.periodic_verdict(outalloc, lo, nelem, item, seven) == ([], 0, 0)
    view[(1 << 32) + 5] = 50.
    assert sk.periodic_verdict(outalloc, lo, nelem, item, seven) == ([], 0, 1)


# ---- decode: float32, float16, bfloat16 -----------------------------------------------------------------

_FLAT_VALUES = {}


def _unit_values(key, small, cidx, pn, coder, bps):
    """float32 (unit, sample) of the compacted units, by launch_expect.decode_values (one slot, rows of 1)."""
    k = (key, pn, coder, bps)
    if k not in _FLAT_VALUES:
        n = len(cidx)
        _FLAT_VALUES[k] = le.decode_values(small, cidx, n, 1, 1, pn, tk.CODERS[coder], bps, False,
                                           fill=(FILL, FILL)).reshape(n, pn * 8 // bps)
    return _FLAT_VALUES[k]


def _interleave(units, nslot, chunk, within=None):
    """Units (frame * nslot + slot, sample) -> (frame, row, slot, chunk or kept positions), as the decode writes."""
    n, E = units.shape
    v = units.reshape(n // nslot, nslot, E // chunk, chunk).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(v if within is None else v[..., list(within)])


def _decode_kernel(nslot, chunk, flat_kernel, out, bps, indexed):
    if out != 'f32':
        return ('k_decode_half_flat<{},' if nslot == 1 else 'k_decode_half_rows<{}>').format(bps)
    if nslot == 1:
        return flat_kernel
    return 'k_decode_gather<' if indexed and (nslot <= 4 or chunk < 32) else 'k_decode_rows_pipe<'


def _decode_forms(inbuf, outalloc, coder, bps, nslot, chunk, out, flat_kernel=None, within=None, staged=False,
                  select_kernel=None):
    """The three forms for one decode geometry: sparse sources, the fixed stride, the dense output."""
    import torch
    from baseband_amd import kernels
    from test_decode_guard_gpu import knobs
    cid = tk.CODERS[coder]
    wdev = None if within is None else torch.tensor(list(within), dtype=torch.int32, device='cuda')
    kw = dict(chunk=chunk, nslot=nslot, fill_value=FILL, out_dtype=_tdtype(out))
    if within is not None:
        kw['within'] = wdev
    what = (coder, bps, nslot, chunk, out, within, staged)
    ran = 0
    with knobs(VDIF8_LDS_GIB=0 if staged else None):
        # 1. sparse sources through an index: frame f, slot s takes place (f * nslot + s) mod 11
        sp = _sparse(inbuf, PN, 100 * bps + nslot)
        nplace = len(sp.at)
        take = np.arange(nplace * nslot) % nplace
        units = _unit_values(('sparse', 100 * bps + nslot), sp.small, sp.cidx, PN, coder, bps)[take]
        want = le.as_out_type(_interleave(units, nslot, chunk, within), out)
        dsrc = torch.from_numpy(sp.index()[take]).cuda()
        kernel = select_kernel or _decode_kernel(nslot, chunk, flat_kernel, out, bps, True)
        _small(outalloc, out, want,
               lambda view: kernels.decode_frames(inbuf, nplace, PN, cid, bps, src=dsrc, out=view, **kw), kernel, what + ('sparse',))
        ran += 1
        # 2. the fixed stride (the selecting kernels work through an index: the wrapper makes it of the stride)
        st = _strided(inbuf)
        units = _unit_values('stride', st.small, st.cidx, PN_STRIDE, coder, bps)
        want = le.as_out_type(_interleave(units, nslot, chunk, within), out)
        kernel = select_kernel or _decode_kernel(nslot, chunk, flat_kernel, out, bps, False)
        _small(outalloc, out, want,
               lambda view: kernels.decode_frames(inbuf, STRIDE_N // nslot, PN_STRIDE, cid, bps, src0=STRIDE_SRC0,
                                                  src_stride=sk.STRIDE, out=view, **kw), kernel, what + ('stride',))
        ran += 1
        # 3. the dense output: live frame sets at the output's seams, their slots at the seam places in turn
        E = PN * 8 // bps
        frame = nslot * (E if within is None else E // chunk * len(within))
        nframes = sk.OUT_ELEMS // frame
        seams = sk.out_seams(_item(out), nframes * frame)
        live = sk.live_frames(frame, nframes, seams)
        valid = sp.valid()
        idx, used = sk.dense_index(nframes, nslot, live, [sp.at[k] for k in valid])
        flat = _unit_values(('sparse', 100 * bps + nslot), sp.small, sp.cidx, PN, coder, bps)
        expect = [(f * frame, le.as_out_type(_interleave(flat[[valid[j] for j in used[f]]], nslot, chunk, within), out))
                  for f in live]
        assert len(live) == 3 * len(seams) and any(a < s < a + e.size for s in seams for a, e in expect)
        dsrc = torch.from_numpy(idx).cuda()
        kernel = select_kernel or _decode_kernel(nslot, chunk, flat_kernel, out, bps, True)
        _dense(outalloc, out, nframes * frame, FILL, expect,
               lambda view: kernels.decode_frames(inbuf, nframes, PN, cid, bps, src=dsrc, out=view, **kw), kernel, what + ('dense',))
        ran += 1
    return ran


def test_decode_float32_flat(inbuf, outalloc):
    ran = 0
    for coder, bps, staged, kernel in FLAT:
        ran += _decode_forms(inbuf, outalloc, coder, bps, 1, 1, 'f32', kernel, staged=staged)
    assert ran == 3 * CASE_COUNTS['FLAT']


def test_decode_float32_thread_shapes(inbuf, outalloc):
    ran = 0
    for coder, bps in WIDTHS:
        for nslot, chunk in SHAPES:
            ran += _decode_forms(inbuf, outalloc, coder, bps, nslot, chunk, 'f32')
    assert ran == 3 * CASE_COUNTS['WIDTHS'] * CASE_COUNTS['SHAPES']


def test_decode_float32_selections(inbuf, outalloc):
    ran = 0
    for coder, bps in (('vdif', 2), ('int', 8)):
        for nslot, chunk, within, kernel in SELECTS:
            ran += _decode_forms(inbuf, outalloc, coder, bps, nslot, chunk, 'f32', within=within, select_kernel=kernel)
    assert ran == 3 * 2 * CASE_COUNTS['SELECTS']


def test_decode_sources_past_2_to_the_33(outalloc):
    """The decode family once more with sparse sources in a buffer of 2^33 + 2^26 bytes: the places around 2^32
    and 2^33 (the module's own input buffer ends short of those)."""
    import torch
    from baseband_amd import kernels
    size = (1 << 33) + sk.TAIL
    _need(size + (1 << 30))
    big = torch.empty(size, dtype=torch.uint8, device='cuda')
    ran = 0
    for coder, bps, nslot, chunk, out, kernel in BEYOND:
        sp = sk.Sparse(big, PN, sk.places(PN, size, low=1 << 32, high=1 << 33), np.random.default_rng(40 + ran))
        assert max(sp.at) > 1 << 33 and len(sp.valid()) == 9
        small, cidx = sp.compact()
        nplace = len(sp.at)
        take = np.arange(nplace * nslot) % nplace
        units = le.decode_values(small, cidx, nplace, 1, 1, PN, tk.CODERS[coder], bps, False, fill=(FILL, FILL))
        want = le.as_out_type(_interleave(units.reshape(nplace, -1)[take], nslot, chunk), out)
        dsrc = torch.from_numpy(sp.index()[take]).cuda()
        _small(outalloc, out, want,
               lambda view: kernels.decode_frames(big, nplace, PN, tk.CODERS[coder], bps, chunk=chunk, nslot=nslot, src=dsrc,
                                                  fill_value=FILL, out=view, out_dtype=_tdtype(out)), kernel, (coder, bps, nslot, out))
        ran += 1
    assert ran == CASE_COUNTS['BEYOND']
    del big


def test_decode_half(inbuf, outalloc):
    ran = 0
    for out, coder, bps in HALF:
        ran += _decode_forms(inbuf, outalloc, coder, bps, 1, 1, out)
        ran += _decode_forms(inbuf, outalloc, coder, bps, HALF_SHAPE[0], HALF_SHAPE[1], out)
    assert ran == 6 * CASE_COUNTS['HALF']


# ---- Mark 4 ------------------------------------------------------------------------------------------------

def test_mark4(inbuf, outalloc):
    import torch
    from baseband_amd import kernels
    from test_decode_guard_gpu import knobs
    ran = 0
    for ntrack, widen, fill_words, select in MARK4:
        perm = np.random.default_rng(ntrack + widen).permutation(ntrack)
        sign, mag = [int(x) for x in perm[:ntrack // 2]], [int(x) for x in perm[ntrack // 2:]]
        if select:
            sign, mag = sign[:3], mag[:3]
        nout, wbytes, r = len(sign), ntrack // 8, 64 // ntrack
        what = (ntrack, widen, fill_words, select)

        def kernel(nwords):
            wide = bool(widen) and r > 1 and nwords % r == 0 and fill_words % r == 0 and nout * r <= 32
            return 'k_decode_mark4{}<{},'.format('_select' if select else '', 64 if wide else ntrack)

        kw = dict(fill_words=fill_words, fill_value=M4_FILL, select=select)
        with knobs(M4_WIDEN=widen):
            # 1. sparse sources
            unit = M4_WORDS * wbytes
            sp = _sparse(inbuf, unit, 1000 + ntrack, align=8)
            want = le.mark4_values(sp.small, sp.cidx, len(sp.at), ntrack, M4_WORDS, sign, mag, fill_words, fill=M4_FILL)
            dsrc = torch.from_numpy(sp.index()).cuda()
            _small(outalloc, 'f32', want,
                   lambda view: kernels.decode_mark4(inbuf, len(sp.at), ntrack, M4_WORDS, sign, mag, src=dsrc, out=view, **kw),
                   kernel(M4_WORDS), what + ('sparse',))
            # 2. the fixed stride
            st = _strided(inbuf)
            want = le.mark4_values(st.small, st.cidx, STRIDE_N, ntrack, M4_WORDS_STRIDE, sign, mag, fill_words, fill=M4_FILL)
            _small(outalloc, 'f32', want,
                   lambda view: kernels.decode_mark4(inbuf, STRIDE_N, ntrack, M4_WORDS_STRIDE, sign, mag, src0=STRIDE_SRC0,
                                                     src_stride=sk.STRIDE, out=view, **kw),
                   kernel(M4_WORDS_STRIDE), what + ('stride',))
            # 3. the dense output
            frame = M4_WORDS * nout
            nframes = sk.OUT_ELEMS // frame
            seams = sk.out_seams(4, nframes * frame)
            live = sk.live_frames(frame, nframes, seams)
            valid = sp.valid()
            idx, used = sk.dense_index(nframes, 1, live, [sp.at[k] for k in valid])
            ref = le.mark4_values(sp.small, sp.cidx, len(sp.at), ntrack, M4_WORDS, sign, mag, fill_words, fill=M4_FILL)
            expect = [(f * frame, ref[valid[used[f][0]]]) for f in live]
            dsrc = torch.from_numpy(idx).cuda()
            _dense(outalloc, 'f32', nframes * frame, M4_FILL, expect,
                   lambda view: kernels.decode_mark4(inbuf, nframes, ntrack, M4_WORDS, sign, mag, src=dsrc, out=view, **kw),
                   kernel(M4_WORDS), what + ('dense',))
        ran += 3
    assert ran == 3 * CASE_COUNTS['MARK4']


# ---- int8 transposes -------------------------------------------------------------------------------------------

def test_i8_transposes_at_the_fixed_stride(inbuf, outalloc):
    import torch
    from baseband_amd import kernels
    st = _strided(inbuf)
    fill = complex(*TILED_FILL)
    ran = 0
    for layout, npol, nchan, ntime in XPOSE:
        assert ntime * npol * nchan * 2 <= STRIDE_UNIT
        want = le.tiled_values(st.small, st.cidx, STRIDE_N, layout, npol, nchan, ntime, 0, ntime, fill=TILED_FILL)
        _small(outalloc, 'f32', want,
               lambda view: kernels.decode_i8_tiled(inbuf, STRIDE_N, layout, npol, nchan, ntime, 0, ntime, src0=STRIDE_SRC0,
                                                    src_stride=sk.STRIDE, fill_value=fill, out=view),
               'k_decode_i8_xpose<{},'.format(layout), ('xpose', layout))
        ran += 1
    assert ran == CASE_COUNTS['XPOSE']
    # a channel list and the second of two polarisations
    cmap = torch.tensor(PICK_CHANNELS, dtype=torch.int32, device='cuda')
    ran = 0
    for layout, ntime, kernel in XPOSE_PICK:
        assert ntime * 2 * PICK_STORED * 2 <= STRIDE_UNIT
        t_lo, t_hi = 8, ntime - 3
        want = le.tiled_values(st.small, st.cidx, STRIDE_N, layout, 1, len(PICK_CHANNELS), ntime, t_lo, t_hi,
                               nchan_stored=PICK_STORED, npol_stored=2, pol_first=1, chan_map=PICK_CHANNELS, fill=TILED_FILL)
        _small(outalloc, 'f32', want,
               lambda view: kernels.decode_i8_tiled(inbuf, STRIDE_N, layout, 1, len(PICK_CHANNELS), ntime, t_lo, t_hi,
                                                    src0=STRIDE_SRC0, src_stride=sk.STRIDE, fill_value=fill, out=view,
                                                    nchan_stored=PICK_STORED, npol_stored=2, pol_first=1, chan_map=cmap),
               kernel, ('pick', layout))
        ran += 1
    assert ran == CASE_COUNTS['XPOSE_PICK']


def test_i8_transposes_through_an_index(inbuf, outalloc):
    import torch
    from baseband_amd import kernels
    fill = complex(*TILED_FILL)
    ran = 0
    for layout, npol, nchan, ntime, kernel in TILED:
        unit = ntime * npol * nchan * 2
        sp = _sparse(inbuf, unit, 2000 + layout, align=2)
        n = len(sp.at)
        ref = le.tiled_values(sp.small, sp.cidx, n, layout, npol, nchan, ntime, 0, ntime, fill=TILED_FILL)
        dsrc = torch.from_numpy(sp.index()).cuda()
        _small(outalloc, 'f32', ref,
               lambda view: kernels.decode_i8_tiled(inbuf, n, layout, npol, nchan, ntime, 0, ntime, src=dsrc, fill_value=fill,
                                                    out=view), kernel, ('tiled', layout, 'sparse'))
        nframes = sk.OUT_ELEMS // unit                      # (a float per payload byte)
        seams = sk.out_seams(4, nframes * unit)
        live = sk.live_frames(unit, nframes, seams)
        valid = sp.valid()
        idx, used = sk.dense_index(nframes, 1, live, [sp.at[k] for k in valid])
        expect = [(f * unit, ref[valid[used[f][0]]]) for f in live]
        dsrc = torch.from_numpy(idx).cuda()
        _dense(outalloc, 'f32', nframes * unit, FILL, expect,
               lambda view: kernels.decode_i8_tiled(inbuf, nframes, layout, npol, nchan, ntime, 0, ntime, src=dsrc,
                                                    fill_value=fill, out=view), kernel, ('tiled', layout, 'dense'))
        ran += 1
    assert ran == CASE_COUNTS['TILED']


# ---- encoders ------------------------------------------------------------------------------------------------------

def _periodic_floats(nelem, block):
    """float32 device tensor of `nelem` elements: the NumPy `block` over and over."""
    import torch
    x = torch.empty(nelem, dtype=torch.float32, device='cuda')
    assert x.data_ptr() % 16 == 0
    tile = torch.from_numpy(block).cuda().repeat((256 << 20) // block.nbytes)
    for a in range(0, nelem, tile.numel()):
        n = min(tile.numel(), nelem - a)
        x[a:a + n] = tile[:n]
    return x


def _encode_into(outalloc, nbytes, first_bytes, call, kernel, what):
    """`call(view)` writes `nbytes` bytes into a view of the poisoned allocation, judged as 32-bit words that
    repeat `first_bytes`.  `kernel` None: the entry leaves no note of its kernel."""
    from baseband_amd import _lib
    assert nbytes % 4 == 0 and first_bytes.size % 4 == 0
    first = np.ascontiguousarray(first_bytes).view(np.uint32)
    assert not guardkit.contains_poison(first), what
    lo, view = _view(outalloc, nbytes // 4, 'f32')
    call(view)
    note = _lib.last_kernel()
    v = sk.periodic_verdict(outalloc, lo, nbytes // 4, 4, first)
    assert guardkit.clean(v), (what, note, guardkit.describe(v, nbytes // 4))
    assert kernel is None or note.startswith(kernel), (what, note, kernel)


def test_encoders_past_2_to_the_32_elements(outalloc):
    import ctypes as C
    import torch
    import encode_steps as es
    from baseband_amd import kernels, _lib
    _need(4 * ENCODE_ELEMS + (2 << 30))
    st = kernels.current_stream(torch.device('cuda'))
    ran = 0
    for coder, bps in ENCODES:
        noise = np.random.default_rng(bps).standard_normal(ENCODE_PERIOD).astype(np.float32)
        block = es.mixed_input(coder, bps, noise, 3 + bps)
        first = es.oracle_packed(block, coder, bps)
        x = _periodic_floats(ENCODE_ELEMS, block)
        nbytes = ENCODE_ELEMS * bps // 8
        _encode_into(outalloc, nbytes, first,
                     lambda view: kernels.check(_lib.lib.bb_encode_flat(C.c_void_p(x.data_ptr()), ENCODE_ELEMS, tk.CODERS[coder], bps,
                                                                        C.c_void_p(view.data_ptr()), nbytes, st), 'bb_encode_flat'),
                     'k_encode_flat<VDIF,{},'.format(bps), (coder, bps))
        del x
        ran += 1
    assert ran == CASE_COUNTS['ENCODES']
    ran = 0
    for ntrack in ENCODES_M4:
        opw = ntrack // 2
        perm = np.random.default_rng(ntrack).permutation(ntrack)
        sign, mag = [int(v) for v in perm[:opw]], [int(v) for v in perm[opw:]]
        noise = np.random.default_rng(ntrack).standard_normal(2 * ENCODE_PERIOD).astype(np.float32)      # 8191 words of 64 tracks
        block = es.mixed_input('vdif', 2, noise, 5 + ntrack)
        first = es.mark4_encode_np(block, ntrack, sign, mag)
        x = _periodic_floats(ENCODE_ELEMS, block)
        nwords = ENCODE_ELEMS // opw
        nbytes = nwords * ntrack // 8
        u8 = C.c_uint8 * 32
        _encode_into(outalloc, nbytes, np.asarray(first).view(np.uint8),
                     lambda view: kernels.check(_lib.lib.bb_encode_mark4(C.c_void_p(x.data_ptr()), nwords, ntrack, u8(*sign), u8(*mag),
                                                                         C.c_void_p(view.data_ptr()), nbytes, st), 'bb_encode_mark4'),
                     'k_encode_mark4<{},'.format(ntrack), ('mark4', ntrack))
        del x
        ran += 1
    assert ran == CASE_COUNTS['ENCODES_M4']


# ---- the packed-byte family (these entries leave no note of the kernel: the entry called is the kernel's) ------------

PACKED_IN = (2, 2, 4, 1040)         # bits, slots, codes per row and slot, payload bytes of the sparse and strided requests
# entry -> (bits out, (slots, chunk) out, payload out): frames of 1000 bytes do not line up with the input's
PACKED_OUT = {'repack': (2, (4, 2), 1000), 'requant': (4, (2, 4), 1000), 'recode': (8, (8, 1), 1000)}
PACKED_BIG = (1 << 29) + 64         # one 1-bit payload: bit offsets and row numbers past 2^32
# entry -> (bits out, code map) of the big payload: outputs of 2^29, 2^30 and 2^31 bytes (and a little)
BIG_OUT = {'repack': (1, (1, 0)), 'requant': (2, (2, 1)), 'recode': (4, (9, 6))}
FIRST_ROWS = [('requant', 2, 8, (1, 1), (1, 1)), ('requant', 2, 4, (1, 1), (1, 1)), ('repack', 8, 8, (1, 1), (1, 1)),
              ('recode', 2, 8, (2, 1), (1, 2))]
CASE_COUNTS.update(PACKED_OUT=3, BIG_OUT=3, FIRST_ROWS=4)


def _state_counts(req, nslot, chunk, bps, row_lo, row_hi, bin_rows=None, first_row=0, nbins=None):
    """Counts of the raw codes of rows [row_lo, row_hi) of a recodekit.Request: (slot, position, code), or with
    `bin_rows` (slot, bin, position, code)."""
    rows, valid = req.rows[row_lo:row_hi], req.valid[row_lo:row_hi]
    nlev = 1 << bps
    out = np.zeros((nslot, chunk, nlev) if bin_rows is None else (nslot, nbins, chunk, nlev), np.int64)
    b = None if bin_rows is None else (first_row + np.arange(len(rows), dtype=np.int64)) // bin_rows
    for s in range(nslot):
        for c in range(chunk):
            col = s * chunk + c
            v = valid[:, col]
            if bin_rows is None:
                out[s, c] = np.bincount(rows[v, col], minlength=nlev)
            else:
                out[s, :, c, :] = np.bincount(b[v] * nlev + rows[v, col], minlength=nbins * nlev).reshape(nbins, nlev)
    return out


def _packed_call(entry, dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table, out, **kw):
    from baseband_amd import kernels, _lib
    (ns_i, ch_i), (ns_o, ch_o) = shape_in, shape_out
    if entry == 'repack':
        assert bps_in == bps_out
        coder_out = _lib.CODER_MARK5B if bps_in <= 2 else _lib.CODER_VDIF
        return kernels.repack_frames(dbuf, nframes, payload_in, bps_in, _lib.CODER_VDIF, ch_i, ns_i, coder_out, ch_o, ns_o,
                                     payload_out, out=out, **kw)
    if entry == 'requant':
        assert shape_in == shape_out
        return kernels.requant_frames(dbuf, nframes, payload_in, bps_in, ch_i, ns_i, bps_out, payload_out, table, out=out, **kw)
    return kernels.recode_frames(dbuf, nframes, payload_in, bps_in, ch_i, ns_i, bps_out, ch_o, ns_o, payload_out, table,
                                 out=out, **kw)


def _table(entry, bps_in, bps_out, seed):
    """The code map: VDIF -> Mark 5B for the repack (1 bit: inverted, 2 bits: the two bits swapped; 8 bits: VDIF ->
    VDIF, the identity), a random one otherwise."""
    if entry == 'repack':
        return np.array({1: [1, 0], 2: [0, 2, 1, 3]}.get(bps_in, list(range(1 << bps_in))), np.uint8)
    import recodekit
    return recodekit.random_table(np.random.default_rng(seed), bps_in, bps_out)


def _packed_small(outalloc, entry, dbuf, req, nframes, payload_in, bps_in, shape_in, row_lo, row_hi, first_row, what, **src):
    """One launch of an output entry into a small poisoned view, judged as packedkit.judge judges."""
    import torch
    import packedkit
    import recodekit
    bps_out, shape_out, payload_out = PACKED_OUT[entry]
    if entry == 'repack':
        bps_out = bps_in
    table = _table(entry, bps_in, bps_out, 7)
    nbytes = recodekit.nbytes_out(row_hi - row_lo, first_row, bps_out, shape_out, payload_out)
    guardkit.refill(outalloc)
    lo = guardkit.GUARD // 4
    view = outalloc[lo:lo + nbytes // 4]
    before = np.tile(np.array([guardkit.POISON], np.uint32).view(np.uint8), nbytes // 4)
    want = req.expect(before, table, bps_out, shape_out, payload_out, 1, row_lo, row_hi, first_row)
    got = _packed_call(entry, dbuf, nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table,
                       view.view(torch.uint8), fill_code=1, row_lo=row_lo, row_hi=row_hi, first_row=first_row, **src)
    assert got.data_ptr() == view.data_ptr()
    packedkit.judge(outalloc[:(2 * guardkit.GUARD + nbytes) // 4], view, want, what)


def _packed_forms(inbuf, outalloc, ref_buf, ref_src, nframes, what, **src):
    """count_states, count_states_bins and the three output entries on one source, all against one Request."""
    import recodekit
    from baseband_amd import kernels
    bps, nslot, chunk, payload = PACKED_IN
    req = recodekit.Request(ref_buf, ref_src, nframes, payload, bps, nslot, chunk)
    assert req.valid.any()
    total = req.total
    row_lo, row_hi, first_row = 8, total - 16, 24
    got = kernels.count_states(inbuf, nframes, payload, bps, chunk, nslot, row_lo=row_lo, row_hi=row_hi, **src)
    assert np.array_equal(got.cpu().numpy(), _state_counts(req, nslot, chunk, bps, row_lo, row_hi)), what
    bin_rows = 1000
    nbins = (first_row + row_hi - row_lo - 1) // bin_rows + 1
    got = kernels.count_states_bins(inbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins, row_lo=row_lo, row_hi=row_hi,
                                    first_row=first_row, **src)
    assert np.array_equal(got.cpu().numpy(), _state_counts(req, nslot, chunk, bps, row_lo, row_hi, bin_rows, first_row, nbins)), what
    ran = 0
    for entry in PACKED_OUT:
        _packed_small(outalloc, entry, inbuf, req, nframes, payload, bps, (nslot, chunk), row_lo, row_hi, first_row,
                      what + (entry,), **src)
        ran += 1
    assert ran == CASE_COUNTS['PACKED_OUT']


def test_packed_sparse_sources_and_the_fixed_stride(inbuf, outalloc):
    import torch
    bps, nslot, chunk, payload = PACKED_IN
    st = _strided(inbuf)
    sp = _sparse(inbuf, payload, 3000)
    nplace = len(sp.at)
    take = np.arange(nplace * nslot) % nplace
    _packed_forms(inbuf, outalloc, sp.small, sp.cidx[take], nplace, ('sparse',),
                  src=torch.from_numpy(sp.index()[take]).cuda())
    _packed_forms(inbuf, outalloc, st.small, st.cidx, STRIDE_N // nslot, ('stride',), src0=STRIDE_SRC0, src_stride=sk.STRIDE)


def _ones(block, a, b):
    """Set bits in bytes [a, b) of a buffer that repeats the NumPy `block`."""
    cum = np.concatenate([[0], np.cumsum(np.unpackbits(block).reshape(-1, 8).sum(1), dtype=np.int64)])

    def upto(x):
        return (x // block.size) * int(cum[-1]) + int(cum[x % block.size])
    return upto(b) - upto(a)


def test_packed_payload_with_bit_offsets_past_32_bits(inbuf, outalloc):
    """One 1-bit payload of 2^29 + 64 bytes (rows are bits: 2^32 + 512 of them), periodic: the whole of it, and
    the rows [2^32 - 8000, 2^32 + 256) alone."""
    import torch
    import recodekit
    from baseband_amd import kernels
    P = PACKED_BIG
    block = _periodic_input(inbuf, P, BIG_PERIOD, 31)
    src = dict(src0=0, src_stride=P)
    ranges = [(0, 8 * P), ((1 << 32) - 8000, (1 << 32) + 256)]
    for row_lo, row_hi in ranges:
        ones = _ones(block, row_lo // 8, row_hi // 8)
        got = kernels.count_states(inbuf, 1, P, 1, 1, 1, row_lo=row_lo, row_hi=row_hi, **src)
        assert got.cpu().numpy().reshape(2).tolist() == [row_hi - row_lo - ones, ones], (row_lo, row_hi)
        # bins of 2^31 - 8 rows: the third begins short of row 2^32
        bin_rows = (1 << 31) - 8
        nbins = 3
        want = np.zeros((nbins, 2), np.int64)
        for k in range(nbins):
            a, b = max(row_lo, k * bin_rows), min(row_hi, (k + 1) * bin_rows)
            if a < b:
                want[k, 1] = _ones(block, a // 8, b // 8)
                want[k, 0] = b - a - want[k, 1]
        got = kernels.count_states_bins(inbuf, 1, P, 1, 1, 1, bin_rows, nbins, row_lo=row_lo, row_hi=row_hi, first_row=row_lo, **src)
        assert np.array_equal(got.cpu().numpy().reshape(nbins, 2), want), (row_lo, row_hi)
    # the three output entries: the whole payload (periodic output) ...
    one = recodekit.Request(block, [0], 1, block.size, 1, 1, 1)
    ran = 0
    for entry, (bps_out, table) in BIG_OUT.items():
        table = np.array(table, np.uint8)
        first = one.expect(np.zeros(block.size * bps_out, np.uint8), table, bps_out, (1, 1), block.size * bps_out, 0)
        nbytes = P * bps_out
        _encode_into(outalloc, nbytes, first,
                     lambda view: _packed_call(entry, inbuf, 1, P, 1, (1, 1), bps_out, (1, 1), nbytes, table, view.view(torch.uint8),
                                               **src), None, (entry, 'whole'))
        # ... and the rows either side of row 2^32, into a small output
        row_lo, row_hi = ranges[1]
        near = inbuf[row_lo // 8:row_hi // 8].cpu().numpy()
        req = recodekit.Request(near, [0], 1, near.size, 1, 1, 1)
        nb = (row_hi - row_lo) * bps_out // 8
        guardkit.refill(outalloc)
        lo = guardkit.GUARD // 4
        view = outalloc[lo:lo + nb // 4]
        want = req.expect(np.zeros(nb, np.uint8), table, bps_out, (1, 1), nb, 0)
        _packed_call(entry, inbuf, 1, P, 1, (1, 1), bps_out, (1, 1), nb, table, view.view(torch.uint8), row_lo=row_lo,
                     row_hi=row_hi, **src)
        import packedkit
        packedkit.judge(outalloc[:(2 * guardkit.GUARD + nb) // 4], view, want, (entry, 'rows at 2^32'))
        ran += 1
    assert ran == CASE_COUNTS['BIG_OUT']


def test_packed_first_row_at_the_output_seams(outalloc):
    """`first_row` = 2^32 - 4096: the written rows straddle output row 2^32, and with it output byte 2^31 (4-bit
    rows), 2^32 (one byte per row) or 2^33 (two).  Everything else of the output stays poison."""
    import torch
    import packedkit
    import recodekit
    ran = 0
    for entry, bps_in, bps_out, shape_in, shape_out in FIRST_ROWS:
        rng = np.random.default_rng(bps_out + len(entry))
        (ns_i, ch_i), (ns_o, ch_o) = shape_in, shape_out
        nframes, payload_in = 3, 4096 * ch_i * bps_in // 8          # 4096 rows in a frame
        buf, src = packedkit.indexed_case(rng, payload_in, nframes, ns_i)
        req = recodekit.Request(buf, src, nframes, payload_in, bps_in, ns_i, ch_i)
        table = _table(entry, bps_in, bps_out, 13)
        payload_out = 3 << 20                                       # frames that do not end on a power of two
        R_out = payload_out * 8 // bps_out // ch_o
        first_row, nrows = (1 << 32) - 4096, req.total
        nbytes = recodekit.nbytes_out(nrows, first_row, bps_out, shape_out, payload_out)
        assert nbytes <= 4 * sk.OUT_ELEMS and first_row % R_out and (first_row + nrows) // R_out == first_row // R_out
        guardkit.refill(outalloc)
        lo = guardkit.GUARD // 4
        view = outalloc[lo:lo + nbytes // 4]
        _packed_call(entry, packedkit.device(buf), nframes, payload_in, bps_in, shape_in, bps_out, shape_out, payload_out, table,
                     view.view(torch.uint8), fill_code=1, src=packedkit.device(src), first_row=first_row)
        # the output frame that holds the rows, against the oracle; the rest by a count of what is no longer poison
        F = first_row // R_out
        a, b = F * ns_o * payload_out, (F + 1) * ns_o * payload_out
        before = np.tile(np.array([guardkit.POISON], np.uint32).view(np.uint8), (b - a) // 4)
        want = req.expect(before, table, bps_out, shape_out, payload_out, 1, 0, nrows, first_row - F * R_out)
        got = view[a // 4:b // 4].cpu().numpy().view(np.uint8)
        assert np.array_equal(got, want), (entry, bps_out, int((got != want).sum()))
        changed = int((want.view(np.uint32) != guardkit.POISON).sum())
        assert changed >= nrows * ch_o * bps_out // 32 * ns_o - 8
        left = 0
        for c in range(0, nbytes // 4, sk.CHUNK):
            left += sk._poison_count(view[c:c + sk.CHUNK], 0, 4)
        assert nbytes // 4 - left == changed, (entry, bps_out, "stores outside the rows asked for")
        assert sk.guards_touched(outalloc, lo, nbytes // 4, 4) == []
        ran += 1
    assert ran == CASE_COUNTS['FIRST_ROWS']


def test_bins_longer_than_32_bits_of_bytes():
    """Bins of 2^28 + 8 rows of 16 bytes (`bin_bytes` 2^32 + 128) and a `first_row` in bin 16, past row 2^32."""
    import packedkit
    import recodekit
    from baseband_amd import kernels
    bps, chunk, nslot, payload, nframes = 2, 64, 1, 16384, 4
    rng = np.random.default_rng(17)
    buf = rng.integers(0, 256, nframes * payload, dtype=np.uint8)
    src = np.arange(nframes, dtype=np.int64) * payload
    req = recodekit.Request(buf, src, nframes, payload, bps, nslot, chunk)
    bin_rows = (1 << 28) + 8
    assert bin_rows * chunk * bps // 8 > 1 << 32
    first_row = 17 * bin_rows - 1024
    nbins = 18
    got = kernels.count_states_bins(packedkit.device(buf), nframes, payload, bps, chunk, nslot, bin_rows, nbins,
                                    src0=0, src_stride=payload, first_row=first_row)
    want = _state_counts(req, nslot, chunk, bps, 0, req.total, bin_rows, first_row, nbins)
    assert want[0, 16].sum() == 1024 * chunk and want[0, 17].sum() == (req.total - 1024) * chunk
    assert np.array_equal(got.cpu().numpy(), want)


# ---- scans and searches ----------------------------------------------------------------------------------------------

SCANS = ['vdif', 'mark5b', 'mark4']
SCAN_PAD = 256
CASE_COUNTS.update(SCANS=3)


def scan_runs(F, seams=(sk.LOW, sk.HIGH)):
    """Starts of the runs of three frames of `F` bytes (a multiple of 8) planted around each seam: one at every
    residue mod 4, the third straddling the seam with its first frame, none within a frame of another."""
    assert F % 8 == 0
    return [s + d for s in seams for d in (-9 * F, -4 * F - F // 2 + 1, -F // 2 + 2, 3 * F + F // 2 + 3)]


class _Planted:
    """Frames of one format in a zeroed input buffer, and the same frames back to back in a small NumPy buffer."""

    def __init__(self, inbuf, kind):
        import bb_index_np as ix
        _Buffers.strided = None
        inbuf.zero_()
        self.kind, self.ix, self.size = kind, ix, int(inbuf.shape[0])
        self.F = {'vdif': 8032, 'mark5b': ix.M5B_FRAME, 'mark4': 16 * 2500}[kind]
        self.head = {'vdif': 32, 'mark5b': 16, 'mark4': 0}[kind]       # from a frame's start to what its record points at
        self.runs = scan_runs(self.F)
        assert sorted(q % 4 for q in self.runs[:4]) == [0, 1, 2, 3] and self.runs[2] < sk.LOW < self.runs[2] + self.F
        self.frames = [q + k * self.F for q in self.runs for k in range(3)]
        for j, p in enumerate(self.frames):
            sk._write(inbuf, p, self.header(j))
        if kind == 'mark5b':                                        # one frame of the fill pattern: INVALID
            self.fill_at = self.frames[-1]
            sk._write(inbuf, self.fill_at + 16, np.tile(ix.words_to_bytes([ix.M5B_FILL]), (self.F - 16) // 4))
        self.inbuf = inbuf

    def header(self, j):
        ix = self.ix
        if self.kind == 'vdif':
            return ix.words_to_bytes(ix.vdif_header_words(self.F, 32, seconds=100 + j // 5, frame_nr=j % 5, thread_id=j % 3,
                                                          invalid=int(j == 7)))
        if self.kind == 'mark5b':
            return ix.words_to_bytes(ix.mark5b_header_words(frame_nr=j % 7, jday=123, seconds=4000 + j // 7, user=0x1234))
        return ix.mark4_header_stream(16, uyear=5, day=10, sec=j)

    def pattern(self):
        return self.ix.vdif_header_words(self.F, 32), self.ix.VDIF_MASKS['edv0']

    def compact(self, offsets):
        """-> (small, offsets there): the frames at `offsets` back to back, then the buffer's last F - 4 bytes, so
        that an offset whose frame ends outside the buffer keeps its distance from the end."""
        F = self.F
        small = np.zeros(len(offsets) * F + F - 4, np.uint8)
        small[len(offsets) * F:] = sk._read(self.inbuf, self.size - (F - 4), self.size)
        at = []
        for k, p in enumerate(offsets):
            if p + F <= self.size:
                small[k * F:(k + 1) * F] = sk._read(self.inbuf, p, p + F)
                at.append(k * F)
            else:
                at.append(small.size - (self.size - p))
        return small, at

    def records(self, small, at):
        ix = self.ix
        if self.kind == 'vdif':
            pattern, mask = self.pattern()
            return ix.vdif_records(small, at, self.F, 32, pattern, mask, 100, 0, 5)
        if self.kind == 'mark5b':
            return ix.mark5b_records(small, at, 123 * 86400 + 4000, 0, 7)
        return ix.mark4_records(small, at, 16, 2015, 10 * 86400 * 4000, 4000)

    def scan_at(self, offsets):
        import torch
        from baseband_amd import kernels
        dev = torch.tensor(offsets, dtype=torch.int64, device='cuda')
        if self.kind == 'vdif':
            pattern, mask = self.pattern()
            return kernels.vdif_scan_at(self.inbuf, self.size, dev, self.F, 32, pattern, mask, 100, 0, 5)
        if self.kind == 'mark5b':
            return kernels.mark5b_scan_at(self.inbuf, self.size, dev, 123 * 86400 + 4000, 0, 7)
        return kernels.mark4_scan_at(self.inbuf, self.size, dev, 16, 2015, 10 * 86400 * 4000, 4000)

    def locates(self):
        """What every search entry of the format finds in the whole buffer: lists of offsets."""
        import ctypes as C
        from baseband_amd import kernels, _lib
        if self.kind == 'vdif':
            pattern, mask = self.pattern()
            return [kernels.vdif_locate(self.inbuf, self.size, self.F, 32, pattern, mask).tolist()]
        if self.kind == 'mark5b':
            plain = kernels._collect_offsets(
                lambda offs, cap, count: _lib.lib.bb_mark5b_locate(kernels._ptr(self.inbuf), self.size, offs, cap, count,
                                                                   kernels._stream(self.inbuf)),
                self.inbuf, self.size // self.F + 16, 'bb_mark5b_locate')
            return [plain.tolist(), kernels.mark5b_locate(self.inbuf, self.size, 0x12340000, 0xffff0000).tolist()]
        return [kernels.mark4_locate(self.inbuf, self.size, 16).tolist()]

    def oracle_locates(self, buf):
        ix = self.ix
        if self.kind == 'vdif':
            pattern, mask = self.pattern()
            return [ix.vdif_locate(buf, self.F, 32, pattern, mask).tolist()]
        if self.kind == 'mark5b':
            return [ix.mark5b_locate(buf).tolist(), ix.mark5b_locate(buf, 0x12340000, 0xffff0000).tolist()]
        return [ix.mark4_locate(buf, 16).tolist()]


def test_scans_and_searches_either_side_of_the_seams(inbuf):
    from baseband_amd import kernels
    ran = 0
    for kind in SCANS:
        pl = _Planted(inbuf, kind)
        F = pl.F
        # records at the planted frames, at places that hold zeros, and at one whose frame ends outside the buffer
        offsets = pl.frames + [sk.LOW + 64 * F, sk.HIGH + 64 * F + 4, pl.size - F, pl.size - F + 4]
        small, at = pl.compact(offsets)
        want = pl.records(small, at)
        got = kernels.recs_fields(pl.scan_at(offsets))
        assert got['payload_offset'].tolist() == [p + pl.head for p in offsets], kind
        assert want['payload_offset'].tolist() == [a + pl.head for a in at]
        for key in ('time_index', 'thread_id', 'flags'):
            assert got[key].tolist() == want[key].tolist(), (kind, key)
        ok = (want['flags'] & 1).tolist()
        assert ok == [1] * len(pl.frames) + [0, 0, 0, 0], (kind, ok)
        assert want['time_index'].tolist()[:len(pl.frames)] == list(range(len(pl.frames))), kind
        assert (want['flags'] >> 1 & 1).sum() == (0 if kind == 'mark4' else 1), kind
        # searches over the whole buffer: exactly what the oracle confirms in windows around the runs
        expect = None
        for q in pl.runs:
            lo, hi = q - SCAN_PAD, q + 3 * F + SCAN_PAD
            found = pl.oracle_locates(sk._read(inbuf, lo, hi))
            expect = [e + [lo + p for p in f] for e, f in zip(expect, found)] if expect else [[lo + p for p in f] for f in found]
        zeros = pl.oracle_locates(np.zeros(3 * F + 2 * SCAN_PAD, np.uint8))
        for got_list, exp_list, z in zip(pl.locates(), expect, zeros):
            assert z == [], (kind, "zero bytes are a candidate")
            assert got_list == sorted(exp_list), (kind, got_list, sorted(exp_list))
            assert exp_list == [q + k * F for q in pl.runs for k in (0, 1)], kind
            assert min(exp_list) < sk.LOW < exp_list[5] and exp_list[7] < sk.HIGH < max(exp_list)
        ran += 1
    assert ran == CASE_COUNTS['SCANS']


# ---- periodic data: copies, single payloads past the seams ------------------------------------------------------

def _periodic_input(inbuf, nbytes, period, seed):
    """A random block of `period` bytes over and over in the first `nbytes` of the input buffer (the units at
    the fixed stride are gone after this).  -> the block (NumPy)."""
    import torch
    _Buffers.strided = None
    block = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8)
    words = block[:period // 4 * 4].view(np.uint32)
    words[words == guardkit.POISON] = 0
    tile = torch.from_numpy(block).cuda().repeat((64 << 20) // period)
    for a in range(0, nbytes, tile.numel()):
        n = min(tile.numel(), nbytes - a)
        inbuf[a:a + n] = tile[:n]
    return block


def test_copy_fixed_stride(inbuf, outalloc):
    from baseband_amd import kernels
    st = _strided(inbuf)
    ran = 0
    for form, width in COPIES:
        n = STRIDE_UNIT if width == 16 else STRIDE_UNIT - 4
        want = le.copy_values(st.small, STRIDE_N, n, 0, STRIDE_UNIT)
        _small(outalloc, 'f32', want,
               lambda view: kernels.copy_frames(inbuf, STRIDE_N, n, src0=STRIDE_SRC0, src_stride=sk.STRIDE, out=view),
               'k_copy_frames<nt,{},'.format(form), (form, 'stride'))
        ran += 1
    assert ran == CASE_COUNTS['COPIES']


def _periodic(outalloc, nelem, out, first, launch, kernel, what):
    from baseband_amd import _lib
    assert not guardkit.contains_poison(first), what
    lo, view = _view(outalloc, nelem, out)
    res = launch(view)
    note = _lib.last_kernel()
    assert res.data_ptr() == view.data_ptr(), (what, "a temporary stood in")
    v = sk.periodic_verdict(outalloc, lo, nelem, _item(out), first)
    assert guardkit.clean(v), (what, note, guardkit.describe(v, nelem))
    assert note.startswith(kernel), (what, note, kernel)
    return lo, view


def test_copy_output_seams_and_a_run_past_32_bits(inbuf, outalloc):
    """Every run the same `n` bytes (stride 0), `n` an odd prime number of rows: the output is periodic and its
    byte offsets pass 2^31 .. 2^34; then one run of 2^32 + 2^20 bytes of periodic input."""
    from baseband_amd import kernels
    ran = 0
    for form, width in COPIES:
        n = COPY_PERIOD * width
        block = _periodic_input(inbuf, 1 << 20, n, 5 + width)
        nframes = 4 * sk.OUT_ELEMS // n
        assert nframes * n > 1 << 34 and all(s % n for s in (1 << 31, 1 << 32, 1 << 33, 1 << 34))
        _periodic(outalloc, nframes * n // 4, 'f32', block.view(np.float32),
                  lambda view: kernels.copy_frames(inbuf, nframes, n, src0=0, src_stride=0, out=view),
                  'k_copy_frames<nt,{},'.format(form), (form, 'seams'))
        ran += 1
    assert ran == CASE_COUNTS['COPIES']
    nbytes = (1 << 32) + (1 << 20)
    block = _periodic_input(inbuf, nbytes, BIG_PERIOD, 9)
    _periodic(outalloc, nbytes // 4, 'f32', block.view(np.float32),
              lambda view: kernels.copy_frames(inbuf, 1, nbytes, src0=0, src_stride=nbytes, out=view),
              'k_copy_frames<nt,16B,', 'one run')


def test_one_payload_past_the_seams(inbuf, outalloc):
    """('int', 8) with one payload of 2^32 + 2^20 bytes, ('int', 4) with one of 2^31 + 2^20: offsets inside one
    payload past 32 bits.  First period against NumPy, the whole output against a torch expression, in pieces."""
    import torch
    from baseband_amd import kernels, _lib
    ran = 0
    for coder, bps, pn, out, kernel in BIG_PAYLOADS:
        block = _periodic_input(inbuf, pn, BIG_PERIOD, 20 + bps)
        first = le.as_out_type(orc.decode_flat(block, coder, bps), out)
        nelem = pn * 8 // bps
        lo, view = _periodic(outalloc, nelem, out, first,
                             lambda view: kernels.decode_frames(inbuf, 1, pn, tk.CODERS[coder], bps, src0=0, src_stride=pn,
                                                                fill_value=FILL, out=view, out_dtype=_tdtype(out)),
                             kernel, (coder, bps, pn, out))
        levels = torch.from_numpy(_lib.get_levels(tk.CODERS[coder], bps).astype(np.float32)).cuda()
        step = 1 << 26                                      # input bytes per piece
        for a in range(0, pn, step):
            b = inbuf[a:min(pn, a + step)]
            if bps == 8:
                want = b.view(torch.int8).to(_tdtype(out))
            else:
                want = levels[torch.stack((b & 15, b >> 4), 1).reshape(-1).long()].to(_tdtype(out))
            got = view[a * 8 // bps:a * 8 // bps + want.numel()]
            ity = torch.int32 if out == 'f32' else torch.int16
            assert torch.equal(got.view(ity), want.view(ity)), (coder, bps, out, a)
        ran += 1
    assert ran == CASE_COUNTS['BIG_PAYLOADS']
