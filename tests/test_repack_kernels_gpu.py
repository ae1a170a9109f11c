"""bb_repack_frames on the device against the same permutation of bit fields done with
NumPy on the bytes alone: exact byte equality.  Every slot shape at every width it has,
frames that do not line up, coder pairs, payloads through an index (shuffled, odd
addresses, missing, negative, out of bounds) and at a fixed stride, row ranges with a
first row, one request split over two calls, more work items than a workgroup takes, and
every argument error.  Outputs are poisoned and guarded: bytes outside the rows written
must still hold the poison.  A second, independent pin on a subset: the package's own
decode followed by its encode."""
import ctypes

import numpy as np
import pytest

import guardkit
from packedkit import _torch, unpack_codes, pack_codes, device, whole_rows, indexed_case, judge

pytestmark = pytest.mark.gpu

VDIF, MARK5B, INT = 0, 1, 2
# the code maps, written out: MAPS[(coder_in, coder_out)][bps][code]
IDENT = {bps: list(range(1 << bps)) for bps in (1, 2, 4, 8)}
MAPS = {(VDIF, VDIF): IDENT, (MARK5B, MARK5B): {1: [0, 1], 2: [0, 1, 2, 3]}, (INT, INT): {4: IDENT[4], 8: IDENT[8]},
        (VDIF, MARK5B): {1: [1, 0], 2: [0, 2, 1, 3]}, (MARK5B, VDIF): {1: [1, 0], 2: [0, 2, 1, 3]}}
FILL_CODE = {(VDIF, 1): 1, (VDIF, 2): 2, (MARK5B, 1): 0, (MARK5B, 2): 1}   # what 0.0 encodes to
# (nslot, chunk) in -> out
SHAPES = [((1, 8), (1, 8)), ((8, 1), (1, 8)), ((1, 8), (8, 1)), ((2, 2), (4, 1)), ((16, 1), (1, 16)),
          ((32, 1), (2, 16)), ((1, 1), (1, 1))]
CASES = [(i, o, bps) for i, o in SHAPES for bps in (1, 2, 4, 8) if i[0] * i[1] * bps <= 256]
PAYLOADS = ((40, 37), (104, 19), (8000, 5))                 # (bytes, frames); rounded up to whole rows


def pairs_of(bps):
    return [pair for pair, maps in sorted(MAPS.items()) if bps in maps]


def byte_unit(bps, chunk_in, chunk_out):
    """Rows between byte boundaries common to every input and output slot stream."""
    return max(1, 8 // (bps * min(chunk_in, chunk_out)))


class Request:
    """The codes of every row of a request, by component (NumPy, from the bytes alone)."""

    def __init__(self, buf, src, nframes, payload_in, bps, shape_in):
        self.bps, (self.nslot_in, self.chunk_in) = bps, shape_in
        self.R_in = R = payload_in * 8 // bps // self.chunk_in
        self.total = nframes * R
        ncomp = self.nslot_in * self.chunk_in
        self.codes = np.zeros((nframes, R, ncomp), np.uint8)
        self.valid = np.zeros((nframes, R, ncomp), bool)
        for f in range(nframes):
            for s in range(self.nslot_in):
                so = int(src[f * self.nslot_in + s])
                if so < 0 or so + payload_in > len(buf):
                    continue
                k = slice(s * self.chunk_in, (s + 1) * self.chunk_in)
                self.codes[f, :, k] = unpack_codes(buf[so:so + payload_in], bps).reshape(R, self.chunk_in)
                self.valid[f, :, k] = True
        self.codes = self.codes.reshape(self.total, ncomp)
        self.valid = self.valid.reshape(self.total, ncomp)

    def expect(self, before, pair, shape_out, payload_out, fill_code, row_lo=0, row_hi=None, first_row=0):
        """`before` (the output buffer's bytes, whole output frames) with the rows of the
        request written into it."""
        bps = self.bps
        nslot_out, chunk_out = shape_out
        row_hi = self.total if row_hi is None else row_hi
        R_out = payload_out * 8 // bps // chunk_out
        nout = len(before) // (nslot_out * payload_out)
        assert nout * nslot_out * payload_out == len(before)
        out = unpack_codes(before, bps).reshape(nout, nslot_out, R_out, chunk_out).copy()
        table = np.array(MAPS[pair][bps], np.uint8)
        c = np.where(self.valid[row_lo:row_hi], table[self.codes[row_lo:row_hi]], np.uint8(fill_code))
        G = first_row + np.arange(row_hi - row_lo)
        assert G.size == 0 or G[-1] // R_out < nout
        out[G // R_out, :, G % R_out, :] = c.reshape(len(G), nslot_out, chunk_out)
        return pack_codes(out, bps)


def nbytes_out(nrows, first_row, bps, shape_out, payload_out):
    R_out = payload_out * 8 // bps // shape_out[1]
    return -(-(first_row + nrows) // R_out) * shape_out[0] * payload_out


def run(dbuf, nframes, payload_in, bps, pair, shape_in, shape_out, payload_out, fill_code, nout_bytes, **kw):
    """One launch into a poisoned, guarded output -> (whole, view, bytes before the launch)."""
    from baseband_amd import kernels
    torch = _torch()
    whole, view = guardkit.poisoned(nout_bytes // 4, torch.int32)
    before = view.cpu().numpy().view(np.uint8).copy()
    out = view.view(torch.uint8)
    got = kernels.repack_frames(dbuf, nframes, payload_in, bps, pair[0], shape_in[1], shape_in[0], pair[1],
                                shape_out[1], shape_out[0], payload_out, fill_code=fill_code, out=out, **kw)
    assert got is out
    return whole, view, before


def payloads_out(payload_in, bps, shape_in, shape_out):
    """Output payloads whose frames do not line up with the input's, and one that does."""
    per_frame = payload_in * shape_in[0] // shape_out[0]     # the bytes of an input frame's rows, per output slot
    unit = max(4, shape_out[1] * bps // 8)
    return sorted({whole_rows(32, bps, shape_out[1]), whole_rows(64, bps, shape_out[1]),
                   whole_rows(per_frame, bps, shape_out[1]) + unit, whole_rows(payload_in, bps, shape_out[1])})


@pytest.mark.parametrize('shape_in,shape_out,bps', CASES)
def test_repack_through_an_index(shape_in, shape_out, bps):
    rng = np.random.default_rng(100 * bps + 10 * shape_in[0] + shape_out[0])
    u = byte_unit(bps, shape_in[1], shape_out[1])
    for nbytes, nframes in PAYLOADS:
        payload_in = whole_rows(nbytes, bps, shape_in[1])
        buf, src = indexed_case(rng, payload_in, nframes, shape_in[0])
        dbuf, dsrc = device(buf), device(src)
        req = Request(buf, src, nframes, payload_in, bps, shape_in)
        assert req.valid.any() and not req.valid.all()
        hi = req.total // u * u
        for payload_out in payloads_out(payload_in, bps, shape_in, shape_out):
            for pair in pairs_of(bps):
                fill = int(rng.integers(0, 1 << bps))
                n = nbytes_out(hi, 0, bps, shape_out, payload_out)
                whole, view, before = run(dbuf, nframes, payload_in, bps, pair, shape_in, shape_out, payload_out,
                                          fill, n, src=dsrc, row_hi=hi)
                want = req.expect(before, pair, shape_out, payload_out, fill, 0, hi)
                judge(whole, view, want, (payload_in, nframes, payload_out, pair))


@pytest.mark.parametrize('shape_in,shape_out,bps', CASES)
def test_repack_at_a_fixed_stride(shape_in, shape_out, bps):
    rng = np.random.default_rng(200 * bps + 10 * shape_in[0] + shape_out[0])
    u = byte_unit(bps, shape_in[1], shape_out[1])
    for nbytes, nframes in PAYLOADS:
        payload_in = whole_rows(nbytes, bps, shape_in[1])
        src0, stride = 8, payload_in + 4                    # (every other payload off the 16-byte grid)
        n = nframes * shape_in[0]
        buf = rng.integers(0, 256, src0 + (n - 1) * stride + payload_in, dtype=np.uint8)
        dbuf = device(buf)
        req = Request(buf, src0 + np.arange(n) * stride, nframes, payload_in, bps, shape_in)
        assert req.valid.all()
        hi = req.total // u * u
        pair = pairs_of(bps)[-1]
        for payload_out in payloads_out(payload_in, bps, shape_in, shape_out):
            nb = nbytes_out(hi, 0, bps, shape_out, payload_out)
            whole, view, before = run(dbuf, nframes, payload_in, bps, pair, shape_in, shape_out, payload_out, 0, nb,
                                      src0=src0, src_stride=stride, row_hi=hi)
            judge(whole, view, req.expect(before, pair, shape_out, payload_out, 0, 0, hi), (payload_in, payload_out))


@pytest.mark.parametrize('shape_in,shape_out,bps', CASES)
def test_row_ranges_with_a_first_row(shape_in, shape_out, bps):
    """Ranges that begin and end inside frames, in one frame, without the first and last
    frames and empty, placed anywhere in the output."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(300 * bps + 10 * shape_in[0] + shape_out[0])
    nframes = 7
    payload_in = whole_rows(260, bps, shape_in[1])
    buf, src = indexed_case(rng, payload_in, nframes, shape_in[0])
    dbuf, dsrc = device(buf), device(src)
    req = Request(buf, src, nframes, payload_in, bps, shape_in)
    u = byte_unit(bps, shape_in[1], shape_out[1])
    R, total = req.R_in, req.total // u * u
    ranges = [(3 * u, total - 5 * u), (u, 2 * u), (R // u * u + u, R // u * u + 2 * u), (2 * R // u * u, 3 * R // u * u - u),
              (R // u * u, total - R // u * u), (total - u, total)]
    pair = pairs_of(bps)[-1]
    for k, (lo, hi) in enumerate(ranges):
        assert 0 <= lo < hi <= total
        for payload_out in payloads_out(payload_in, bps, shape_in, shape_out)[1:]:
            R_out = payload_out * 8 // bps // shape_out[1]
            for first_row in (0, 5 * u, R_out // u * u - u, 3 * (R_out // u * u) + u):
                n = nbytes_out(hi - lo, first_row, bps, shape_out, payload_out) + (k & 1) * shape_out[0] * payload_out
                whole, view, before = run(dbuf, nframes, payload_in, bps, pair, shape_in, shape_out, payload_out, 1, n,
                                          src=dsrc, row_lo=lo, row_hi=hi, first_row=first_row)
                want = req.expect(before, pair, shape_out, payload_out, 1, lo, hi, first_row)
                judge(whole, view, want, (lo, hi, payload_out, first_row))
    # an empty range and a request of no frames write nothing
    payload_out = payloads_out(payload_in, bps, shape_in, shape_out)[0]
    for lo, nf in ((0, nframes), (9 * u, nframes), (total, nframes), (0, 0)):
        whole, view, before = run(dbuf, nf, payload_in, bps, pair, shape_in, shape_out, payload_out, 0,
                                  shape_out[0] * payload_out, src=dsrc, row_lo=lo, row_hi=lo)
        judge(whole, view, before, ('empty', lo, nf))
    # without `out`: whole output frames, as many as the rows need
    got = kernels.repack_frames(dbuf, nframes, payload_in, bps, pair[0], shape_in[1], shape_in[0], pair[1],
                                shape_out[1], shape_out[0], payload_out, src=dsrc, row_lo=u, row_hi=total, first_row=u)
    assert got.dtype == torch.uint8 and got.numel() == nbytes_out(total - u, u, bps, shape_out, payload_out)


@pytest.mark.parametrize('shape_in,shape_out,bps,payload_in,payload_out',
                         [((8, 1), (1, 8), 2, 8000, 5000), ((1, 8), (8, 1), 2, 10000, 1000), ((1, 16), (1, 16), 2, 10000, 8192),
                          ((1, 2), (1, 2), 8, 1000, 1032), ((2, 2), (4, 1), 1, 104, 64), ((16, 1), (1, 16), 4, 4096, 5000)])
def test_a_request_split_over_two_calls(shape_in, shape_out, bps, payload_in, payload_out):
    """Frames [0, k) and [k, n) into one output buffer with the matching first_row: the
    output frame that straddles the cut is completed by the second call, which must not
    disturb a byte of the first call's."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(400 * bps + shape_in[0])
    nframes = 11
    buf, src = indexed_case(rng, payload_in, nframes, shape_in[0])
    dbuf, dsrc = device(buf), device(src)
    req = Request(buf, src, nframes, payload_in, bps, shape_in)
    u = byte_unit(bps, shape_in[1], shape_out[1])
    R = req.R_in
    pair = pairs_of(bps)[-1]
    lo, hi = 3 * u, req.total - 2 * u
    for first_row in (0, 2 * u):
        n = nbytes_out(hi - lo, first_row, bps, shape_out, payload_out)
        for k in (1, 4, 10):
            whole, view, before = run(dbuf, k, payload_in, bps, pair, shape_in, shape_out, payload_out, 1, n,
                                      src=dsrc[:k * shape_in[0]], row_lo=lo, row_hi=k * R, first_row=first_row)
            half = req.expect(before, pair, shape_out, payload_out, 1, lo, k * R, first_row)
            judge(whole, view, half, ('first call', k, first_row))
            kernels.repack_frames(dbuf, nframes - k, payload_in, bps, pair[0], shape_in[1], shape_in[0], pair[1],
                                  shape_out[1], shape_out[0], payload_out, fill_code=1,
                                  src=dsrc[k * shape_in[0]:].contiguous(), row_lo=0, row_hi=hi - k * R,
                                  first_row=first_row + k * R - lo, out=view.view(torch.uint8))
            want = req.expect(before, pair, shape_out, payload_out, 1, lo, hi, first_row)
            judge(whole, view, want, ('both calls', k, first_row))


@pytest.mark.parametrize('shape_in,shape_out,bps,payload_in,payload_out',
                         [((8, 1), (1, 8), 2, 8000, 5032), ((1, 8), (8, 1), 2, 10000, 8000), ((1, 16), (1, 16), 2, 10000, 8192),
                          ((1, 2), (1, 2), 8, 8192, 8000)])
def test_more_work_items_than_a_workgroup_takes(shape_in, shape_out, bps, payload_in, payload_out):
    """Some 200 work items of 8 KiB: on the default grid one per wave with a last workgroup
    that is not full, and on a grid of 3 workgroups (BB_TUNE_BLOCKS) waves that walk many
    items and end at different times."""
    from baseband_amd import _lib, kernels
    rng = np.random.default_rng(500 * bps + shape_in[0])
    nframes = (1600 << 10) // (payload_in * shape_in[0]) + 3
    src0, stride = 0, payload_in
    n = nframes * shape_in[0]
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    req = Request(buf, np.arange(n) * stride, nframes, payload_in, bps, shape_in)
    pair = pairs_of(bps)[-1]
    u = byte_unit(bps, shape_in[1], shape_out[1])
    lo, hi = u, req.total // u * u - 3 * u
    nb = nbytes_out(hi - lo, 0, bps, shape_out, payload_out)
    want = None
    try:
        for blocks in (0, 3):
            kernels.tune(_lib.TUNE_BLOCKS, blocks)
            whole, view, before = run(dbuf, nframes, payload_in, bps, pair, shape_in, shape_out, payload_out, 0, nb,
                                      src0=src0, src_stride=stride, row_lo=lo, row_hi=hi)
            if want is None:
                want = req.expect(before, pair, shape_out, payload_out, 0, lo, hi)
            judge(whole, view, want, ('blocks', blocks))
    finally:
        kernels.tune(_lib.TUNE_BLOCKS, 0)


SECOND_PIN = [(i, o, bps) for i, o, bps in CASES if bps <= 2]


@pytest.mark.parametrize('shape_in,shape_out,bps', SECOND_PIN)
def test_against_decode_then_encode(shape_in, shape_out, bps):
    """The package's own decode of the input followed by its encoder, permuted to the
    output's payload order, gives the same bytes (fill value 0.0, its code from the table)."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(600 * bps + 10 * shape_in[0] + shape_out[0])
    nframes = 6
    payload_in = 1056                                       # 33 x 32: whole dwords on both sides for every shape
    payload_out = payload_in * shape_in[0] // shape_out[0]
    assert payload_out % 4 == 0
    buf, src = indexed_case(rng, payload_in, nframes, shape_in[0])
    dbuf, dsrc = device(buf), device(src)
    R_out = payload_out * 8 // bps // shape_out[1]
    for pair in pairs_of(bps):
        got = kernels.repack_frames(dbuf, nframes, payload_in, bps, pair[0], shape_in[1], shape_in[0], pair[1],
                                    shape_out[1], shape_out[0], payload_out, fill_code=FILL_CODE[pair[1], bps], src=dsrc)
        data = kernels.decode_frames(dbuf, nframes, payload_in, pair[0], bps, shape_in[1], shape_in[0], src=dsrc,
                                     fill_value=0.)
        data = data.reshape(nframes, R_out, shape_out[0], shape_out[1]).permute(0, 2, 1, 3).contiguous()
        want = kernels.encode_flat(data.reshape(-1), pair[1], bps)
        assert got.shape == want.shape and torch.equal(got, want), pair


def test_argument_errors_leave_the_output_untouched():
    from baseband_amd import _lib
    torch = _torch()
    C = ctypes
    rng = np.random.default_rng(7)
    nframes, payload_in, payload_out, bps = 5, 1000, 520, 2
    shape_in, shape_out = (8, 1), (1, 8)
    n = nframes * shape_in[0]
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    dsrc = device(np.arange(n, dtype=np.int64) * payload_in)
    R_in = payload_in * 8 // bps
    total = nframes * R_in
    nb = nbytes_out(total, 0, bps, shape_out, payload_out)
    whole, view = guardkit.poisoned(nb // 4, torch.int32)
    ok = dict(bps=bps, coder_in=VDIF, coder_out=MARK5B, chunk_in=1, nslot_in=8, chunk_out=8, nslot_out=1,
              payload_in=payload_in, payload_out=payload_out, fill_code=1, src0=0, src_stride=payload_in,
              row_lo=0, row_hi=total, first_row=0)

    def call(buf_ptr=dbuf.data_ptr(), buf_n=dbuf.numel(), src_ptr=dsrc.data_ptr(), nfr=nframes,
             out_ptr=view.data_ptr(), out_n=nb, **kw):
        p = _lib.repack_params(**dict(ok, **kw))
        return _lib.lib.bb_repack_frames(buf_ptr, buf_n, src_ptr, nfr, C.byref(p), out_ptr, out_n, None)

    E, R, N = _lib.BB_EINVAL, _lib.BB_ERANGE, _lib.BB_ENOTSUP
    refusals = [
        (E, dict(buf_ptr=None)), (E, dict(out_ptr=None)), (E, dict(buf_ptr=dbuf.data_ptr() + 2)),
        (E, dict(out_ptr=view.data_ptr() + 4)), (E, dict(reserved=1)), (E, dict(payload_in=1002)),
        (E, dict(payload_out=522)), (E, dict(payload_out=0)), (E, dict(row_lo=9, row_hi=8)), (E, dict(chunk_out=4)),
        (E, dict(fill_code=4)), (E, dict(fill_code=-1)),
        (E, dict(bps=8, coder_out=VDIF, chunk_in=2, chunk_out=16, payload_out=40)),       # not whole rows
        (E, dict(src_ptr=None, src0=2)), (E, dict(src_ptr=None, src_stride=-1000)),
        (R, dict(row_hi=total + 4)), (R, dict(out_n=total * 16 // 8 - 1)), (R, dict(first_row=24)),
        (R, dict(src_ptr=None, src_stride=payload_in + 4)), (R, dict(src_ptr=None, src0=4)),
        (N, dict(row_lo=1)), (N, dict(row_hi=total - 2)), (N, dict(first_row=3, row_hi=total - 4)),
        (N, dict(bps=3)), (N, dict(coder_out=INT)), (N, dict(bps=4)), (N, dict(nslot_in=3, chunk_in=8, chunk_out=24)),
        (N, dict(nslot_in=64, chunk_out=64)),
    ]
    for rc, kw in refusals:
        assert call(**kw) == rc, kw
    torch.cuda.synchronize()
    v = guardkit.verdict(whole, view, guardkit.poison_words(nb // 4))
    assert not v.touched and v.wrong == 0 and v.poison_left == nb // 4, guardkit.describe(v, nb // 4)
    # the same block goes through, with an index and at the fixed stride
    req = Request(buf, np.arange(n) * payload_in, nframes, payload_in, bps, shape_in)
    before = view.cpu().numpy().view(np.uint8).copy()
    want = req.expect(before, (VDIF, MARK5B), shape_out, payload_out, 1)
    assert call() == _lib.BB_OK
    judge(whole, view, want, 'index')
    guardkit.refill(whole)
    assert call(src_ptr=None) == _lib.BB_OK
    judge(whole, view, want, 'fixed stride')
