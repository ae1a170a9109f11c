"""bb_count_states_bins on the device against a NumPy count of the same bytes per time
bin: exact equality.  Every geometry the call takes, payloads through an index (shuffled,
odd addresses, missing, out of bounds) and at a fixed stride, bin lengths at every edge
(one byte, bins that straddle frames, one frame, 2.5 frames, 15 / 16 / 17 bytes, one bin
for everything), row ranges with a first row, a request split over two calls,
accumulation between guard words, constant bytes, more work items than waves, 2^17 bins,
and every argument error."""
import ctypes

import numpy as np
import pytest

from packedkit import _torch, unpack_codes, device, whole_rows, indexed_case
from test_states_abi import SUPPORTED
from test_states_kernels_gpu import expected

pytestmark = pytest.mark.gpu

GEOMETRIES = [(bps, chunk) for bps, chunk in SUPPORTED if chunk << bps <= 1024]
PAYLOADS = ((40, 37), (104, 19), (8000, 5))                 # (bytes, frames); rounded up to whole rows
MAX_COUNTERS = 1 << 22                                      # of one expectation


class Codes:
    """Every code of a request, once: its slot, its row in the request and its place
    (position, code) among a bin's counters; sources that count nothing left out."""

    def __init__(self, buf, src, nframes, payload, bps, chunk, nslot):
        self.bps, self.chunk, self.nslot = bps, chunk, nslot
        self.R = R = payload * 8 // bps // chunk
        self.nc = chunk << bps
        self.unit = max(1, 8 // (bps * chunk))              # rows of the shortest legal bin
        e = np.arange(R * chunk)
        slots, rows, places = [], [], []
        for f in range(nframes):
            for s in range(nslot):
                so = int(src[f * nslot + s])
                if so < 0 or so + payload > len(buf):
                    continue
                slots.append(np.full(R * chunk, s, np.int64))
                rows.append(f * R + e // chunk)
                places.append(((e % chunk) << bps) + unpack_codes(buf[so:so + payload], bps))
        self.slot, self.row, self.place = (np.concatenate(x) for x in (slots, rows, places))
        self.total = nframes * R

    def bins(self, bin_rows, nbins, first_row=0, row_lo=0, row_hi=None):
        row_hi = self.total if row_hi is None else row_hi
        m = (self.row >= row_lo) & (self.row < row_hi)
        b = (first_row + self.row[m] - row_lo) // bin_rows
        assert b.size == 0 or b.max() < nbins
        key = (self.slot[m] * nbins + b) * self.nc + self.place[m]
        n = self.nslot * nbins * self.nc
        return np.bincount(key, minlength=n).reshape(self.nslot, nbins, self.chunk, 1 << self.bps)


def bin_lengths(c, nframes):
    """Rows per bin that hit each edge, for a frame of c.R rows."""
    R, unit, cb = c.R, c.unit, c.bps * c.chunk
    odd = unit * (R // unit * 2 // 5 + 1)
    while R % odd == 0:
        odd += unit
    out = {'shortest': unit, 'straddles frames': odd, 'one frame': R,
           '2.5 frames': max(unit, R * 5 // 2 // unit * unit), 'everything': nframes * R}
    for nbytes in (15, 16, 17):
        if nbytes * 8 % cb == 0:
            out['{} bytes'.format(nbytes)] = nbytes * 8 // cb
    return out


def nbins_of(nrows, bin_rows, first_row=0):
    return -(-(first_row + nrows) // bin_rows)


def check_bin_lengths(c, nframes, call):
    for name, bin_rows in bin_lengths(c, nframes).items():
        lo, hi = 0, c.total
        if nbins_of(c.total, bin_rows) * c.nc * c.nslot > MAX_COUNTERS:
            # too many counters for a test: bins around the end of the first frame that counts only
            end = (int(c.row.min()) // c.R + 1) * c.R
            lo, hi = end - 200 * bin_rows, min(c.total, end + 312 * bin_rows)
            assert end - c.R <= lo < end <= hi
        nbins = nbins_of(hi - lo, bin_rows)
        got = call(bin_rows, nbins, row_lo=lo, row_hi=hi)
        assert got.dtype == _torch().int32 and tuple(got.shape) == (c.nslot, nbins, c.chunk, 1 << c.bps)
        want = c.bins(bin_rows, nbins, 0, lo, hi)
        assert want.sum() > 0
        assert np.array_equal(got.cpu().numpy(), want), (name, bin_rows, c.nslot, c.R)
        if name == 'everything':
            assert nbins == 1
            yield got


@pytest.mark.parametrize('bps,chunk', GEOMETRIES)
def test_bins_through_an_index(bps, chunk):
    from baseband_amd import kernels
    rng = np.random.default_rng(1000 * bps + chunk)
    for nslot in (1, 3):
        for nbytes, nframes in PAYLOADS:
            payload = whole_rows(nbytes, bps, chunk)
            buf, src = indexed_case(rng, payload, nframes, nslot)
            dbuf, dsrc = device(buf), device(src)
            c = Codes(buf, src, nframes, payload, bps, chunk, nslot)

            def call(bin_rows, nbins, **kw):
                return kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins,
                                                 src=dsrc, **kw)

            for one_bin in check_bin_lengths(c, nframes, call):
                # one bin holding the whole request: bb_count_states of the same call
                whole = kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src=dsrc)
                assert np.array_equal(one_bin[:, 0].cpu().numpy(), whole.cpu().numpy())
                assert np.array_equal(whole.cpu().numpy(), expected(buf, src, nframes, payload, bps, chunk, nslot))


@pytest.mark.parametrize('bps,chunk', GEOMETRIES)
def test_bins_at_a_fixed_stride(bps, chunk):
    from baseband_amd import kernels
    rng = np.random.default_rng(2000 * bps + chunk)
    for nslot in (1, 3):
        for nbytes, nframes in PAYLOADS:
            payload = whole_rows(nbytes, bps, chunk)
            src0, stride = 8, payload + 4                   # (every other payload off the 16-byte grid)
            n = nframes * nslot
            buf = rng.integers(0, 256, src0 + (n - 1) * stride + payload, dtype=np.uint8)
            dbuf = device(buf)
            c = Codes(buf, src0 + np.arange(n) * stride, nframes, payload, bps, chunk, nslot)

            def call(bin_rows, nbins, **kw):
                return kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins,
                                                 src0=src0, src_stride=stride, **kw)

            for one_bin in check_bin_lengths(c, nframes, call):
                whole = kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src0=src0, src_stride=stride)
                assert np.array_equal(one_bin[:, 0].cpu().numpy(), whole.cpu().numpy())


RANGE_GEOMETRIES = [(1, 1), (1, 4), (2, 1), (2, 2), (4, 1), (2, 16), (8, 2), (8, 4), (1, 128)]


@pytest.mark.parametrize('bps,chunk', RANGE_GEOMETRIES)
def test_row_ranges_with_a_first_row(bps, chunk):
    """Ranges that begin and end inside frames, in one frame, without the first and last
    frames and empty, placed anywhere in the series."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(3000 * bps + chunk)
    nframes, nslot = 7, 2
    payload = whole_rows(260, bps, chunk)
    buf, src = indexed_case(rng, payload, nframes, nslot)
    dbuf, dsrc = device(buf), device(src)
    c = Codes(buf, src, nframes, payload, bps, chunk, nslot)
    R, u, total = c.R, c.unit, c.total
    ranges = [(0, total), (3 * u, total - 5 * u), (u, 2 * u), (R + u, R + 2 * u), (2 * R + 3 * u, 3 * R - u),
              (3 * R - u, 3 * R + u), (R, total - R), (total - u, total)]
    for k, (lo, hi) in enumerate(ranges):
        for bin_rows in (u, 7 * u, R, R + 3 * u):
            for first_row in (0, 5 * u, bin_rows - u, 3 * bin_rows + u):
                nbins = nbins_of(hi - lo, bin_rows, first_row) + (k & 1)      # (a spare bin stays empty)
                got = kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins,
                                                src=dsrc, row_lo=lo, row_hi=hi, first_row=first_row)
                want = c.bins(bin_rows, nbins, first_row, lo, hi)
                assert np.array_equal(got.cpu().numpy(), want), (lo, hi, bin_rows, first_row)
    for lo in (0, 9 * u, total):                            # an empty range adds nothing
        counts = torch.full((nslot, 3, chunk, 1 << bps), 7, dtype=torch.int32, device='cuda')
        assert kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, 8 * u, 3, src=dsrc, row_lo=lo,
                                         row_hi=lo, counts=counts) is counts
        assert bool((counts == 7).all())
    # ... and so does a request of no frames
    counts = torch.zeros((nslot, 3, chunk, 1 << bps), dtype=torch.int32, device='cuda')
    kernels.count_states_bins(dbuf, 0, payload, bps, chunk, nslot, 8 * u, 3, src=dsrc, counts=counts)
    assert int(counts.sum()) == 0


@pytest.mark.parametrize('bps,chunk,payload', [(2, 1, 8000), (2, 16, 10000), (8, 2, 1000), (1, 1, 104), (4, 8, 4096)])
def test_a_request_split_over_two_calls(bps, chunk, payload):
    """Frames [0, k) and [k, n) with the matching first_row: the bin that straddles the
    cut is completed by the second call."""
    from baseband_amd import kernels
    rng = np.random.default_rng(4000 * bps + chunk)
    nframes, nslot = 11, 2
    buf, src = indexed_case(rng, payload, nframes, nslot)
    dbuf, dsrc = device(buf), device(src)
    c = Codes(buf, src, nframes, payload, bps, chunk, nslot)
    R, u = c.R, c.unit
    lo, hi = 3 * u, c.total - 2 * u
    for bin_rows in (u * (R // u * 3 // 7 + 1), 1000 * u, R, 3 * R + u):
        for first_row in (0, 2 * u):
            nbins = nbins_of(hi - lo, bin_rows, first_row)
            one = kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins, src=dsrc,
                                            row_lo=lo, row_hi=hi, first_row=first_row)
            assert np.array_equal(one.cpu().numpy(), c.bins(bin_rows, nbins, first_row, lo, hi))
            for k in (1, 4, 10):
                two = kernels.count_states_bins(dbuf, k, payload, bps, chunk, nslot, bin_rows, nbins,
                                                src=dsrc[:k * nslot], row_lo=lo, row_hi=k * R, first_row=first_row)
                kernels.count_states_bins(dbuf, nframes - k, payload, bps, chunk, nslot, bin_rows, nbins,
                                          src=dsrc[k * nslot:], row_lo=0, row_hi=hi - k * R,
                                          first_row=first_row + k * R - lo, counts=two)
                assert bool((two == one).all()), (bin_rows, first_row, k)


def test_calls_accumulate_and_leave_the_neighbours_alone():
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(5)
    bps, chunk, nslot, payload, nframes = 2, 8, 3, 1000, 6
    buf, src = indexed_case(rng, payload, nframes, nslot)
    dbuf, dsrc = device(buf), device(src)
    c = Codes(buf, src, nframes, payload, bps, chunk, nslot)
    bin_rows = 136
    nbins = nbins_of(c.total, bin_rows)
    n = nslot * nbins * c.nc
    pattern = 0x5a5a5a5a
    big = torch.full((n + 2,), pattern, dtype=torch.int32, device='cuda')      # one guard word on each side
    counts = big[1:1 + n].view(nslot, nbins, chunk, 1 << bps)
    counts.zero_()
    cut = 2 * c.R + 8
    kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins, src=dsrc, row_hi=cut,
                              counts=counts)
    kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins, src=dsrc, row_lo=cut,
                              first_row=cut, counts=counts)
    want = c.bins(bin_rows, nbins)
    assert np.array_equal(counts.cpu().numpy(), want)
    kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins, src=dsrc, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * want)
    assert int(big[0]) == pattern and int(big[-1]) == pattern
    with pytest.raises(TypeError):
        kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, nslot, bin_rows, nbins, src=dsrc,
                                  counts=counts.long())


def byte_table(bps):
    """table[v, c]: how often code c occurs in byte v."""
    return np.stack([np.bincount(unpack_codes([v], bps), minlength=1 << bps) for v in range(256)]).astype(np.uint8)


def test_sum_over_bins_of_4096_frames():
    """More work items than waves in the grid: every run, every flush.  The sum over the
    bins is bb_count_states of the same frames, and the bins are those of NumPy."""
    from baseband_amd import kernels
    nframes, frame, payload = 4096, 8032, 8000
    rng = np.random.default_rng(6)
    buf = rng.integers(0, 256, nframes * frame, dtype=np.uint8)
    dbuf = device(buf)
    bin_rows = 1000
    nbins = nframes * payload * 4 // bin_rows
    got = kernels.count_states_bins(dbuf, nframes, payload, 2, 1, 1, bin_rows, nbins, src0=32, src_stride=frame)
    whole = kernels.count_states(dbuf, nframes, payload, 2, 1, src0=32, src_stride=frame)
    assert bool((got.sum(1, dtype=_torch().int64) == whole).all())
    series = buf.reshape(nframes, frame)[:, 32:].reshape(nbins, bin_rows // 4)
    want = byte_table(2)[series].sum(1, dtype=np.int64)
    assert np.array_equal(got.cpu().numpy().reshape(nbins, 4), want)
    # two interleaved slots of four positions take every other frame each
    nbins //= 8
    got = kernels.count_states_bins(dbuf, nframes // 2, payload, 2, 4, 2, bin_rows, nbins, src0=32, src_stride=frame)
    whole = kernels.count_states(dbuf, nframes // 2, payload, 2, 4, 2, src0=32, src_stride=frame)
    assert bool((got.sum(1, dtype=_torch().int64) == whole).all())
    assert bool((got.sum((2, 3)) == 4 * bin_rows).all())


def test_two_to_the_17_bins_of_64_bytes():
    from baseband_amd import kernels
    nbins, bin_bytes = 1 << 17, 64
    rng = np.random.default_rng(7)
    buf = rng.integers(0, 256, nbins * bin_bytes, dtype=np.uint8)
    dbuf = device(buf)
    want = byte_table(2)[buf.reshape(nbins, bin_bytes)].sum(1, dtype=np.int64)
    for nframes, payload in ((1024, 8192), (1, nbins * bin_bytes), (2048, 4096)):
        got = kernels.count_states_bins(dbuf, nframes, payload, 2, 1, 1, 4 * bin_bytes, nbins, src0=0,
                                        src_stride=payload)
        assert np.array_equal(got.cpu().numpy().reshape(nbins, 4), want), (nframes, payload)


@pytest.mark.parametrize('fill', [0x00, 0xff, 0x1b, (0x44, 0x33, 0x22, 0x11)])
def test_constant_bytes(fill):
    """One byte value throughout (and the Mark 5B fill word): every lane of a wave meets
    the same counters.  Whole, as frames on and off the 16-byte grid; bins shorter than a
    wave's load, of a few loads, and one for everything."""
    from baseband_amd import kernels
    n = 1 << 17
    buf = np.resize(np.atleast_1d(np.array(fill, np.uint8)), n)
    dbuf = device(buf)
    for bps, chunk in ((1, 1), (2, 1), (2, 16), (8, 4)):
        for payload, src0, stride in ((n, 0, 0), (8000, 4, 8004), (4096, 16, 4096)):
            nframes = 1 if stride == 0 else (n - src0) // stride
            c = Codes(buf, src0 + np.arange(nframes) * stride, nframes, payload, bps, chunk, 1)
            for bin_bytes in (16, 48, 100, 252, 1000, 5000, nframes * payload):
                if bin_bytes * 8 % (bps * chunk) or (n // bin_bytes) * c.nc > MAX_COUNTERS:
                    continue
                bin_rows = bin_bytes * 8 // (bps * chunk)
                nbins = nbins_of(c.total, bin_rows)
                got = kernels.count_states_bins(dbuf, nframes, payload, bps, chunk, 1, bin_rows, nbins, src0=src0,
                                                src_stride=stride)
                assert np.array_equal(got.cpu().numpy(), c.bins(bin_rows, nbins)), (bps, chunk, payload, bin_bytes)


def test_argument_errors_leave_the_counts_alone():
    from baseband_amd import _lib, kernels
    torch = _torch()
    bps, chunk, nslot, payload, nframes = 2, 1, 2, 1000, 4
    R = payload * 8 // bps // chunk
    bin_rows, nbins = 1000, 16
    dbuf = torch.zeros(nframes * nslot * payload, dtype=torch.uint8, device='cuda')
    n = nslot * nbins * (chunk << bps)
    counts = torch.full((n + 1,), 3, dtype=torch.int32, device='cuda')

    def call(ncounts=n, counts_ptr=None, stride=payload, buf_nbytes=None, dbuf_off=0, bin_rows=bin_rows, first_row=0,
             nbins=nbins, **kw):
        p = _lib.StatesParams()
        p.bps, p.chunk, p.nslot, p.payload_nbytes = bps, chunk, nslot, payload
        p.src0, p.src_stride = 0, stride
        p.row_lo, p.row_hi = 0, nframes * R
        for k, v in kw.items():
            setattr(p, k, v)
        rc = _lib.lib.bb_count_states_bins(ctypes.c_void_p(dbuf.data_ptr() + dbuf_off),
                                           dbuf.numel() if buf_nbytes is None else buf_nbytes, None, nframes,
                                           ctypes.byref(p), bin_rows, first_row, nbins,
                                           ctypes.c_void_p(counts.data_ptr() if counts_ptr is None else counts_ptr),
                                           ncounts, kernels._stream(dbuf))
        torch.cuda.synchronize()
        return rc

    # BB_EINVAL
    assert call(bin_rows=0) == _lib.BB_EINVAL
    assert call(bin_rows=2 ** 31) == _lib.BB_EINVAL
    assert call(counts_ptr=0) == _lib.BB_EINVAL                 # d_counts NULL
    assert call(counts_ptr=counts.data_ptr() + 2) == _lib.BB_EINVAL            # ... not 4-byte aligned
    assert call(reserved=1) == _lib.BB_EINVAL
    assert call(row_lo=8, row_hi=4) == _lib.BB_EINVAL
    assert call(dbuf_off=2, buf_nbytes=dbuf.numel() - 2, stride=0) == _lib.BB_EINVAL
    assert call(stride=payload + 2, buf_nbytes=1 << 20) == _lib.BB_EINVAL
    # BB_ENOTSUP
    assert call(bin_rows=3) == _lib.BB_ENOTSUP                  # bins are whole bytes
    assert call(bin_rows=1001) == _lib.BB_ENOTSUP
    assert call(bps=8, chunk=8, payload_nbytes=1024) == _lib.BB_ENOTSUP        # 2048 counters per bin
    assert call(bps=8, chunk=16, payload_nbytes=1024) == _lib.BB_ENOTSUP
    assert call(bps=3) == _lib.BB_ENOTSUP
    assert call(first_row=2, nbins=nbins + 1) == _lib.BB_ENOTSUP               # whole bytes only
    assert call(row_lo=1) == _lib.BB_ENOTSUP
    assert call(row_hi=nframes * R - 3) == _lib.BB_ENOTSUP
    # BB_ERANGE
    assert call(ncounts=n - 1) == _lib.BB_ERANGE
    assert call(nbins=nbins - 1) == _lib.BB_ERANGE              # the last counted row's bin
    assert call(first_row=4) == _lib.BB_ERANGE
    assert call(nbins=0, ncounts=0) == _lib.BB_ERANGE
    assert call(row_hi=nframes * R + 4, nbins=nbins + 1, ncounts=n + 1) == _lib.BB_ERANGE
    assert call(stride=payload + 4) == _lib.BB_ERANGE           # the last payload ends outside the buffer
    assert call(buf_nbytes=dbuf.numel() - 1) == _lib.BB_ERANGE
    assert bool((counts == 3).all())
    with pytest.raises(KeyError):
        kernels.count_states_bins(dbuf, nframes, 1024, 8, 8, 1, 1000, 16)
    assert call() == _lib.BB_OK                                 # (the block itself is a good one)
    got = counts[:n].view(nslot, nbins, 4)
    assert bool((got[:, :, 0] == 3 + bin_rows).all()) and bool((got[:, :, 1:] == 3).all()) and int(counts[n]) == 3
    # a bin of the last rows only: the spare room in front stays as it is
    assert call(row_lo=nframes * R - 1000, first_row=1000, nbins=2, ncounts=n) == _lib.BB_OK
    assert int(got[0, 1, 0]) == 3 + 2 * bin_rows and int(got[0, 0, 0]) == 3 + bin_rows
