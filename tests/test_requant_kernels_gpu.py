"""bb_requant_frames on the device against NumPy on the bytes alone: the codes of every
slot stream unpacked at bps_in, sent through the table, packed at bps_out -- exact byte
equality.  All 16 pairs of widths with random tables at every slot shape, frames that do
not line up and frames that do, payloads through an index (shuffled, odd addresses,
missing, negative, out of bounds) and at a fixed stride, row ranges with a first row, one
request split over two calls, more work items than the launch has waves, the identity
table against bb_repack_frames, and every argument error.  Outputs are poisoned and
guarded: bytes outside the rows written must still hold the poison.  `requant_table` is
pinned to the NumPy oracle."""
import ctypes

import numpy as np
import pytest

import guardkit
from packedkit import _torch, unpack_codes, pack_codes, device, whole_rows, indexed_case, judge

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8)
PAIRS = [(bi, bo) for bi in WIDTHS for bo in WIDTHS]
SHAPES = [(1, 1), (1, 8), (8, 1), (2, 2), (16, 1), (32, 1)]     # (nslot, chunk); every row fits 256 bits
PAYLOADS = ((40, 37), (104, 19), (8000, 5))                     # (bytes, frames); rounded up to whole rows


def byte_unit(bps_in, bps_out, chunk):
    """Rows between byte boundaries common to the input and the output slot stream."""
    return max(1, 8 // (chunk * min(bps_in, bps_out)))


def lined_up(nbytes, bps_in, bps_out, chunk):
    """-> (payload_in, payload_out) of the same number of rows, both whole dwords, payload_in >= nbytes."""
    unit = max(1, 32 // (chunk * min(bps_in, bps_out)))
    rows = -(-(nbytes * 8) // (chunk * bps_in * unit)) * unit
    return rows * chunk * bps_in // 8, rows * chunk * bps_out // 8


def payloads_out(payload_lined, bps_out, chunk):
    """Output payloads whose frames do not line up with the input's, and the one that does."""
    unit = max(4, chunk * bps_out // 8)
    return sorted({whole_rows(32, bps_out, chunk), whole_rows(payload_lined + unit, bps_out, chunk),
                   whole_rows(2 * payload_lined // 3, bps_out, chunk), payload_lined})


def random_table(rng, bps_in, bps_out):
    return rng.integers(0, 1 << bps_out, 1 << bps_in, dtype=np.uint8)


class Request:
    """The codes of every slot's stream of a request (NumPy, from the bytes alone)."""

    def __init__(self, buf, src, nframes, payload_in, bps_in, nslot, chunk):
        self.bps_in, self.nslot, self.chunk = bps_in, nslot, chunk
        self.R_in = R = payload_in * 8 // bps_in // chunk
        self.total = nframes * R
        self.codes = np.zeros((nslot, nframes, R * chunk), np.uint8)
        self.valid = np.zeros((nslot, nframes, R * chunk), bool)
        for f in range(nframes):
            for s in range(nslot):
                so = int(src[f * nslot + s])
                if so < 0 or so + payload_in > len(buf):
                    continue
                self.codes[s, f] = unpack_codes(buf[so:so + payload_in], bps_in)
                self.valid[s, f] = True
        self.codes = self.codes.reshape(nslot, -1)
        self.valid = self.valid.reshape(nslot, -1)

    def expect(self, before, table, bps_out, payload_out, fill_code, row_lo=0, row_hi=None, first_row=0):
        """`before` (the output buffer's bytes, whole output frames) with the rows of the
        request written into it."""
        nslot, chunk = self.nslot, self.chunk
        row_hi = self.total if row_hi is None else row_hi
        nout = len(before) // (nslot * payload_out)
        assert nout * nslot * payload_out == len(before)
        out = unpack_codes(before, bps_out).reshape(nout, nslot, -1).transpose(1, 0, 2).reshape(nslot, -1).copy()
        k = slice(row_lo * chunk, row_hi * chunk)
        c = np.where(self.valid[:, k], np.asarray(table, np.uint8)[self.codes[:, k]], np.uint8(fill_code))
        assert (first_row + row_hi - row_lo) * chunk <= out.shape[1]
        out[:, first_row * chunk:(first_row + row_hi - row_lo) * chunk] = c
        return pack_codes(out.reshape(nslot, nout, -1).transpose(1, 0, 2), bps_out)


def nbytes_out(nrows, first_row, bps_out, nslot, chunk, payload_out):
    R_out = payload_out * 8 // bps_out // chunk
    return -(-(first_row + nrows) // R_out) * nslot * payload_out


def run(dbuf, nframes, payload_in, bps_in, shape, bps_out, payload_out, table, fill_code, nout_bytes, **kw):
    """One launch into a poisoned, guarded output -> (whole, view, bytes before the launch)."""
    from baseband_amd import kernels
    torch = _torch()
    whole, view = guardkit.poisoned(nout_bytes // 4, torch.int32)
    before = view.cpu().numpy().view(np.uint8).copy()
    out = view.view(torch.uint8)
    got = kernels.requant_frames(dbuf, nframes, payload_in, bps_in, shape[1], shape[0], bps_out, payload_out, table,
                                 fill_code=fill_code, out=out, **kw)
    assert got is out
    return whole, view, before


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_requant_through_an_index(bps_in, bps_out):
    rng = np.random.default_rng(100 * bps_in + bps_out)
    for nslot, chunk in SHAPES:
        u = byte_unit(bps_in, bps_out, chunk)
        for nbytes, nframes in PAYLOADS:
            payload_in, lined = lined_up(nbytes, bps_in, bps_out, chunk)
            buf, src = indexed_case(rng, payload_in, nframes, nslot)
            dbuf, dsrc = device(buf), device(src)
            req = Request(buf, src, nframes, payload_in, bps_in, nslot, chunk)
            assert req.valid.any() and not req.valid.all()
            hi = req.total // u * u
            for payload_out in payloads_out(lined, bps_out, chunk):
                table = random_table(rng, bps_in, bps_out)
                fill = int(rng.integers(0, 1 << bps_out))
                n = nbytes_out(hi, 0, bps_out, nslot, chunk, payload_out)
                whole, view, before = run(dbuf, nframes, payload_in, bps_in, (nslot, chunk), bps_out, payload_out,
                                          table, fill, n, src=dsrc, row_hi=hi)
                want = req.expect(before, table, bps_out, payload_out, fill, 0, hi)
                judge(whole, view, want, (nslot, chunk, payload_in, nframes, payload_out))


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_requant_at_a_fixed_stride(bps_in, bps_out):
    rng = np.random.default_rng(200 * bps_in + bps_out)
    for nslot, chunk in SHAPES:
        u = byte_unit(bps_in, bps_out, chunk)
        for nbytes, nframes in PAYLOADS[1:]:
            payload_in, lined = lined_up(nbytes, bps_in, bps_out, chunk)
            src0, stride = 8, payload_in + 4                    # (every other payload off the 16-byte grid)
            n = nframes * nslot
            buf = rng.integers(0, 256, src0 + (n - 1) * stride + payload_in, dtype=np.uint8)
            dbuf = device(buf)
            req = Request(buf, src0 + np.arange(n) * stride, nframes, payload_in, bps_in, nslot, chunk)
            assert req.valid.all()
            hi = req.total // u * u
            table = random_table(rng, bps_in, bps_out)
            for payload_out in payloads_out(lined, bps_out, chunk)[1:]:
                nb = nbytes_out(hi, 0, bps_out, nslot, chunk, payload_out)
                whole, view, before = run(dbuf, nframes, payload_in, bps_in, (nslot, chunk), bps_out, payload_out,
                                          table, 0, nb, src0=src0, src_stride=stride, row_hi=hi)
                judge(whole, view, req.expect(before, table, bps_out, payload_out, 0, 0, hi),
                      (nslot, chunk, payload_in, payload_out))


@pytest.mark.parametrize('bps_in,bps_out', PAIRS)
def test_row_ranges_with_a_first_row(bps_in, bps_out):
    """Ranges that begin and end inside frames, in one frame, without the first and last
    frames and empty, placed anywhere in the output."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(300 * bps_in + bps_out)
    nframes = 7
    for nslot, chunk in ((1, 1), (2, 2), (8, 1)):
        payload_in, lined = lined_up(260, bps_in, bps_out, chunk)
        buf, src = indexed_case(rng, payload_in, nframes, nslot)
        dbuf, dsrc = device(buf), device(src)
        req = Request(buf, src, nframes, payload_in, bps_in, nslot, chunk)
        u = byte_unit(bps_in, bps_out, chunk)
        R, total = req.R_in, req.total // u * u
        ranges = [(3 * u, total - 5 * u), (u, 2 * u), (R // u * u + u, R // u * u + 2 * u),
                  (2 * R // u * u, 3 * R // u * u - u), (R // u * u, total - R // u * u), (total - u, total)]
        table = random_table(rng, bps_in, bps_out)
        for k, (lo, hi) in enumerate(ranges):
            assert 0 <= lo < hi <= total
            for payload_out in payloads_out(lined, bps_out, chunk)[1:3]:
                R_out = payload_out * 8 // bps_out // chunk
                for first_row in (0, 5 * u, R_out // u * u - u, 3 * (R_out // u * u) + u):
                    n = nbytes_out(hi - lo, first_row, bps_out, nslot, chunk, payload_out) + (k & 1) * nslot * payload_out
                    whole, view, before = run(dbuf, nframes, payload_in, bps_in, (nslot, chunk), bps_out, payload_out,
                                              table, 1, n, src=dsrc, row_lo=lo, row_hi=hi, first_row=first_row)
                    want = req.expect(before, table, bps_out, payload_out, 1, lo, hi, first_row)
                    judge(whole, view, want, (nslot, chunk, lo, hi, payload_out, first_row))
        # an empty range and a request of no frames write nothing
        payload_out = payloads_out(lined, bps_out, chunk)[0]
        for lo, nf in ((0, nframes), (9 * u, nframes), (total, nframes), (0, 0)):
            whole, view, before = run(dbuf, nf, payload_in, bps_in, (nslot, chunk), bps_out, payload_out, table, 0,
                                      nslot * payload_out, src=dsrc, row_lo=lo, row_hi=lo)
            judge(whole, view, before, ('empty', lo, nf))
        # without `out`: whole output frames, as many as the rows need
        got = kernels.requant_frames(dbuf, nframes, payload_in, bps_in, chunk, nslot, bps_out, payload_out, table,
                                     src=dsrc, row_lo=u, row_hi=total, first_row=u)
        assert got.dtype == torch.uint8 and got.numel() == nbytes_out(total - u, u, bps_out, nslot, chunk, payload_out)


SPLITS = [(8, 2, (1, 1), 8000, 5000), (2, 8, (8, 1), 1000, 1032), (2, 4, (1, 16), 10000, 8192), (1, 8, (2, 2), 104, 64),
          (8, 1, (1, 2), 1000, 104), (2, 2, (1, 1), 1000, 520), (4, 2, (16, 1), 4096, 5000)]


@pytest.mark.parametrize('bps_in,bps_out,shape,payload_in,payload_out', SPLITS)
def test_a_request_split_over_two_calls(bps_in, bps_out, shape, payload_in, payload_out):
    """Frames [0, k) and [k, n) into one output buffer with the matching first_row: the
    output frame that straddles the cut is completed by the second call, which must not
    disturb a byte of the first call's."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(400 * bps_in + bps_out)
    nslot, chunk = shape
    nframes = 11
    buf, src = indexed_case(rng, payload_in, nframes, nslot)
    dbuf, dsrc = device(buf), device(src)
    req = Request(buf, src, nframes, payload_in, bps_in, nslot, chunk)
    u = byte_unit(bps_in, bps_out, chunk)
    R = req.R_in
    assert R % u == 0
    table = random_table(rng, bps_in, bps_out)
    lo, hi = 3 * u, req.total - 2 * u
    for first_row in (0, 2 * u):
        n = nbytes_out(hi - lo, first_row, bps_out, nslot, chunk, payload_out)
        for k in (1, 4, 10):
            whole, view, before = run(dbuf, k, payload_in, bps_in, shape, bps_out, payload_out, table, 1, n,
                                      src=dsrc[:k * nslot], row_lo=lo, row_hi=k * R, first_row=first_row)
            half = req.expect(before, table, bps_out, payload_out, 1, lo, k * R, first_row)
            judge(whole, view, half, ('first call', k, first_row))
            kernels.requant_frames(dbuf, nframes - k, payload_in, bps_in, chunk, nslot, bps_out, payload_out, table,
                                   fill_code=1, src=dsrc[k * nslot:].contiguous(), row_lo=0, row_hi=hi - k * R,
                                   first_row=first_row + k * R - lo, out=view.view(torch.uint8))
            want = req.expect(before, table, bps_out, payload_out, 1, lo, hi, first_row)
            judge(whole, view, want, ('both calls', k, first_row))


@pytest.mark.parametrize('bps_in,bps_out,shape,payload_in,payload_out',
                         [(8, 2, (1, 1), 8000, 5032), (2, 8, (8, 1), 1000, 8000), (2, 4, (1, 16), 10000, 8192),
                          (2, 2, (1, 2), 8192, 8000), (8, 1, (2, 1), 8192, 40000), (1, 8, (1, 1), 1000, 8004)])
def test_more_work_items_than_the_launch_has_waves(bps_in, bps_out, shape, payload_in, payload_out):
    """A few MiB, hundreds of work items: on the default grid one per wave with a last
    workgroup that is not full, and on a grid of 3 workgroups (BB_TUNE_BLOCKS) waves that
    walk many items and end at different times."""
    from baseband_amd import _lib, kernels
    rng = np.random.default_rng(500 * bps_in + bps_out)
    nslot, chunk = shape
    wide = max(bps_in, bps_out) // bps_in                   # so that the wider side has some 2 MiB
    nframes = (2048 << 10) // (payload_in * nslot * wide) + 3
    n = nframes * nslot
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    req = Request(buf, np.arange(n) * payload_in, nframes, payload_in, bps_in, nslot, chunk)
    table = random_table(rng, bps_in, bps_out)
    u = byte_unit(bps_in, bps_out, chunk)
    lo, hi = u, req.total // u * u - 3 * u
    nb = nbytes_out(hi - lo, 0, bps_out, nslot, chunk, payload_out)
    want = None
    try:
        for blocks in (0, 3):
            kernels.tune(_lib.TUNE_BLOCKS, blocks)
            whole, view, before = run(dbuf, nframes, payload_in, bps_in, shape, bps_out, payload_out, table, 0, nb,
                                      src0=0, src_stride=payload_in, row_lo=lo, row_hi=hi)
            if want is None:
                want = req.expect(before, table, bps_out, payload_out, 0, lo, hi)
            judge(whole, view, want, ('blocks', blocks))
    finally:
        kernels.tune(_lib.TUNE_BLOCKS, 0)


@pytest.mark.parametrize('bps', WIDTHS)
def test_the_identity_table_is_a_repack_with_the_identity_map(bps):
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(600 + bps)
    nframes = 9
    for nslot, chunk in ((1, 1), (8, 1), (2, 2), (1, 8)):
        payload_in = whole_rows(1000, bps, chunk)
        buf, src = indexed_case(rng, payload_in, nframes, nslot)
        dbuf, dsrc = device(buf), device(src)
        u = byte_unit(bps, bps, chunk)
        total = nframes * (payload_in * 8 // bps // chunk)
        for payload_out in (whole_rows(520, bps, chunk), payload_in):
            kw = dict(fill_code=1, src=dsrc, row_lo=2 * u, row_hi=total - u, first_row=3 * u)
            want = kernels.repack_frames(dbuf, nframes, payload_in, bps, 0, chunk, nslot, 0, chunk, nslot, payload_out,
                                         out=torch.zeros(nbytes_out(total, 0, bps, nslot, chunk, payload_out),
                                                         dtype=torch.uint8, device='cuda'), **kw)
            got = kernels.requant_frames(dbuf, nframes, payload_in, bps, chunk, nslot, bps, payload_out,
                                         np.arange(1 << bps, dtype=np.uint8), out=torch.zeros_like(want), **kw)
            assert torch.equal(got, want), (nslot, chunk, payload_out)


def test_argument_errors_leave_the_output_untouched():
    from baseband_amd import _lib
    torch = _torch()
    C = ctypes
    rng = np.random.default_rng(7)
    nframes, payload_in, payload_out, bps_in, bps_out, nslot = 5, 1000, 520, 8, 2, 8
    n = nframes * nslot
    buf = rng.integers(0, 256, n * payload_in, dtype=np.uint8)
    dbuf = device(buf)
    dsrc = device(np.arange(n, dtype=np.int64) * payload_in)
    total = nframes * payload_in
    nb = nbytes_out(total, 0, bps_out, nslot, 1, payload_out)
    whole, view = guardkit.poisoned(nb // 4, torch.int32)
    table = random_table(rng, bps_in, bps_out)
    ok = dict(bps_in=bps_in, bps_out=bps_out, chunk=1, nslot=nslot, payload_in=payload_in, payload_out=payload_out,
              table=table, fill_code=1, src0=0, src_stride=payload_in, row_lo=0, row_hi=total, first_row=0)

    def call(buf_ptr=dbuf.data_ptr(), buf_n=dbuf.numel(), src_ptr=dsrc.data_ptr(), nfr=nframes,
             out_ptr=view.data_ptr(), out_n=nb, **kw):
        p = _lib.requant_params(**dict(ok, **kw))
        return _lib.lib.bb_requant_frames(buf_ptr, buf_n, src_ptr, nfr, C.byref(p), out_ptr, out_n, None)

    bad_table = table.copy()
    bad_table[200] = 4
    E, R, N = _lib.BB_EINVAL, _lib.BB_ERANGE, _lib.BB_ENOTSUP
    refusals = [
        (E, dict(buf_ptr=None)), (E, dict(out_ptr=None)), (E, dict(buf_ptr=dbuf.data_ptr() + 2)),
        (E, dict(out_ptr=view.data_ptr() + 4)), (E, dict(reserved=1)), (E, dict(payload_in=1002)),
        (E, dict(payload_out=522)), (E, dict(payload_out=0)), (E, dict(row_lo=12, row_hi=8)),
        (E, dict(fill_code=4)), (E, dict(fill_code=-1)), (E, dict(table=bad_table)),
        (E, dict(chunk=16, payload_in=1000)),                                             # not whole rows
        (E, dict(src_ptr=None, src0=2)), (E, dict(src_ptr=None, src_stride=-1000)),
        (R, dict(row_hi=total + 4)), (R, dict(out_n=total * 2 // 8 * nslot - 1)), (R, dict(first_row=2080)),
        (R, dict(src_ptr=None, src_stride=payload_in + 4)), (R, dict(src_ptr=None, src0=4)),
        (N, dict(row_lo=1)), (N, dict(row_hi=total - 2)), (N, dict(first_row=3, row_hi=total - 4)),
        (N, dict(bps_in=3)), (N, dict(bps_out=3)), (N, dict(nslot=3)), (N, dict(chunk=3)), (N, dict(nslot=64)),
        (N, dict(chunk=64, payload_in=1024)),
    ]
    for rc, kw in refusals:
        assert call(**kw) == rc, kw
    torch.cuda.synchronize()
    v = guardkit.verdict(whole, view, guardkit.poison_words(nb // 4))
    assert not v.touched and v.wrong == 0 and v.poison_left == nb // 4, guardkit.describe(v, nb // 4)
    # the same block goes through, with an index and at the fixed stride
    req = Request(buf, np.arange(n) * payload_in, nframes, payload_in, bps_in, nslot, 1)
    before = view.cpu().numpy().view(np.uint8).copy()
    want = req.expect(before, table, bps_out, payload_out, 1)
    assert call() == _lib.BB_OK
    judge(whole, view, want, 'index')
    guardkit.refill(whole)
    assert call(src_ptr=None) == _lib.BB_OK
    judge(whole, view, want, 'fixed stride')


CODERS = {'vdif': 0, 'mark5b': 1}
ORACLE_PAIRS = [(ci, bi, co, bo) for ci in ('vdif', 'mark5b') for co in ('vdif', 'mark5b')
                for bi in WIDTHS for bo in WIDTHS
                if (ci == 'vdif' or bi <= 2) and (co == 'vdif' or bo <= 2)]


def test_requant_table_is_the_oracles_decode_scale_encode():
    import bb_oracle_np as orc
    from baseband_amd import kernels
    for ci, bi, co, bo in ORACLE_PAIRS:
        levels = np.float32(orc.code_levels(ci, bi))
        for s in (None, 0.5, 2.0, -1.0, 1e-3):
            x = levels if s is None else levels * np.float32(s)
            want = orc.encode_codes(np.float32(x), co, bo)
            got = kernels.requant_table(CODERS[ci], bi, CODERS[co], bo, s)
            assert got.dtype == np.uint8 and got.shape == (1 << bi,)
            assert np.array_equal(got, want), (ci, bi, co, bo, s)
    assert np.array_equal(kernels.requant_table(0, 2, 0, 2, 1.0), kernels.requant_table(0, 2, 0, 2))
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            kernels.requant_table(0, 2, 0, 2, bad)


def test_requant_table_figures():
    """VDIF 8 -> 2 sends the 256 codes to 51 / 77 / 77 / 51 of the four 2-bit codes; VDIF
    2 -> 8 gives codes 10, 92, 163, 245; a scale of 0.5 or 2.0 moves every one of these maps."""
    from baseband_amd import kernels
    down = kernels.requant_table(0, 8, 0, 2)
    assert list(np.bincount(down, minlength=4)) == [51, 77, 77, 51]
    up = kernels.requant_table(0, 2, 0, 8)
    assert list(up) == [10, 92, 163, 245]
    for s in (0.5, 2.0):
        assert not np.array_equal(kernels.requant_table(0, 8, 0, 2, s), down)
        assert not np.array_equal(kernels.requant_table(0, 2, 0, 8, s), up)
