"""bb_count_states on the device against a NumPy count of the same bytes: exact
equality, every width, row width and slot count, payloads through an index (shuffled,
odd addresses, missing, out of bounds) and at a fixed stride, row ranges that begin and
end inside a byte, accumulation, constant bytes, the persistent loop and the 64-bit total."""
import ctypes

import numpy as np
import pytest

from packedkit import _torch, unpack_codes, device, whole_rows, indexed_case

pytestmark = pytest.mark.gpu


def expected(buf, src, nframes, payload, bps, chunk, nslot, row_lo=0, row_hi=None):
    """counts[slot, position, code] of rows [row_lo, row_hi): fields LSB first, a source
    counts only when its whole payload lies inside the buffer."""
    nlev = 1 << bps
    R = payload * 8 // bps // chunk
    row_hi = nframes * R if row_hi is None else row_hi
    out = np.zeros((nslot, chunk, nlev), np.int64)
    pos = (np.arange(R * chunk) % chunk) * nlev
    for f in range(nframes):
        r0, r1 = max(row_lo, f * R) - f * R, min(row_hi, (f + 1) * R) - f * R
        if r0 >= r1:
            continue
        for s in range(nslot):
            so = int(src[f * nslot + s])
            if so < 0 or so + payload > len(buf):
                continue
            key = pos + unpack_codes(buf[so:so + payload], bps)
            out[s] += np.bincount(key[r0 * chunk:r1 * chunk], minlength=chunk * nlev).reshape(chunk, nlev)
    return out


def largest_chunk(bps):
    return 128 // bps


GEOMETRIES = [(bps, chunk) for bps in (1, 2, 4, 8) for chunk in (1, 2, 8, largest_chunk(bps))]
PAYLOADS = ((8, 37), (260, 19), (1000, 11), (8000, 5), (70000, 2))      # (bytes, frames)


@pytest.mark.parametrize('bps,chunk', GEOMETRIES)
def test_counts_through_an_index(bps, chunk):
    from baseband_amd import kernels
    rng = np.random.default_rng(100 * bps + chunk)
    for nslot in (1, 3):
        for nbytes, nframes in PAYLOADS:
            payload = whole_rows(nbytes, bps, chunk)
            buf, src = indexed_case(rng, payload, nframes, nslot)
            got = kernels.count_states(device(buf), nframes, payload, bps, chunk, nslot, src=device(src))
            assert got.dtype == _torch().int64 and tuple(got.shape) == (nslot, chunk, 1 << bps)
            want = expected(buf, src, nframes, payload, bps, chunk, nslot)
            assert want.sum() > 0
            assert np.array_equal(got.cpu().numpy(), want), (nslot, payload)


@pytest.mark.parametrize('bps,chunk', GEOMETRIES)
def test_counts_at_a_fixed_stride(bps, chunk):
    from baseband_amd import kernels
    rng = np.random.default_rng(200 * bps + chunk)
    for nslot in (1, 3):
        for nbytes, nframes in PAYLOADS:
            payload = whole_rows(nbytes, bps, chunk)
            src0, stride = 8, payload + 4                   # (every other payload off the 16-byte grid)
            n = nframes * nslot
            buf = rng.integers(0, 256, src0 + (n - 1) * stride + payload, dtype=np.uint8)
            got = kernels.count_states(device(buf), nframes, payload, bps, chunk, nslot, src0=src0, src_stride=stride)
            want = expected(buf, src0 + np.arange(n) * stride, nframes, payload, bps, chunk, nslot)
            assert np.array_equal(got.cpu().numpy(), want), (nslot, payload)


SUB_BYTE = [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (4, 1)]


@pytest.mark.parametrize('bps,chunk', SUB_BYTE + [(2, 16), (8, 2), (8, 16)])
def test_row_ranges(bps, chunk):
    """Ranges that begin and end inside a byte (rows narrower than one), inside one frame,
    without the first and last frames, and empty."""
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(300 * bps + chunk)
    nframes, nslot = 7, 2
    payload = whole_rows(260, bps, chunk)
    buf, src = indexed_case(rng, payload, nframes, nslot)
    dbuf, dsrc = device(buf), device(src)
    R = payload * 8 // bps // chunk
    total = nframes * R
    ranges = [(0, total), (3, total - 5), (1, 2), (R + 1, R + 2), (2 * R + 3, 3 * R - 1), (3 * R - 1, 3 * R + 1),
              (R, total - R), (R + 5, R + 6), (total - 1, total)]
    for lo, hi in ranges:
        got = kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src=dsrc, row_lo=lo, row_hi=hi)
        want = expected(buf, src, nframes, payload, bps, chunk, nslot, lo, hi)
        assert np.array_equal(got.cpu().numpy(), want), (lo, hi)
    for lo in (0, 9, total):                                # an empty range adds nothing
        counts = torch.full((nslot, chunk, 1 << bps), 7, dtype=torch.int64, device='cuda')
        assert kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src=dsrc, row_lo=lo, row_hi=lo,
                                    counts=counts) is counts
        assert bool((counts == 7).all())
    # ... and so does a request of no frames
    counts = torch.zeros((nslot, chunk, 1 << bps), dtype=torch.int64, device='cuda')
    kernels.count_states(dbuf, 0, payload, bps, chunk, nslot, src=dsrc, counts=counts)
    assert int(counts.sum()) == 0


def test_calls_accumulate_and_leave_the_neighbours_alone():
    from baseband_amd import kernels
    torch = _torch()
    rng = np.random.default_rng(4)
    bps, chunk, nslot, payload, nframes = 2, 8, 3, 1000, 6
    buf, src = indexed_case(rng, payload, nframes, nslot)
    dbuf, dsrc = device(buf), device(src)
    n = nslot * chunk << bps
    pattern = 0x5a5a5a5a5a5a5a5a
    big = torch.full((n + 16,), pattern, dtype=torch.int64, device='cuda')
    counts = big[8:8 + n].view(nslot, chunk, 1 << bps)
    counts.zero_()
    R = payload * 8 // bps // chunk
    kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src=dsrc, row_hi=2 * R + 7, counts=counts)
    kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src=dsrc, row_lo=2 * R + 7, counts=counts)
    want = expected(buf, src, nframes, payload, bps, chunk, nslot)
    assert np.array_equal(counts.cpu().numpy(), want)
    kernels.count_states(dbuf, nframes, payload, bps, chunk, nslot, src=dsrc, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * want)
    assert bool((big[:8] == pattern).all()) and bool((big[8 + n:] == pattern).all())


@pytest.mark.parametrize('fill', [0x00, 0xff, 0x1b, (0x44, 0x33, 0x22, 0x11)])
def test_constant_bytes(fill):
    """1 MiB of one byte value (and of the Mark 5B fill word): every lane of a wave meets
    the same bins.  Whole, as frames on and off the 16-byte grid, for every number of byte
    phases."""
    from baseband_amd import kernels
    n = 1 << 20
    buf = np.resize(np.atleast_1d(np.array(fill, np.uint8)), n)
    dbuf = device(buf)
    for bps, chunk in ((1, 1), (2, 1), (2, 16), (8, 8), (8, 16)):
        for payload, src0, stride in ((n, 0, 0), (8000, 4, 8004), (4096, 16, 4096)):
            nframes = 1 if stride == 0 else (n - src0) // stride
            got = kernels.count_states(dbuf, nframes, payload, bps, chunk, src0=src0, src_stride=stride)
            want = expected(buf, src0 + np.arange(nframes) * stride, nframes, payload, bps, chunk, 1)
            assert np.array_equal(got.cpu().numpy(), want), (bps, chunk, payload)


def test_4096_frames_at_a_fixed_stride():
    """The persistent loop and the flush of every workgroup: more work items than waves."""
    from baseband_amd import kernels
    nframes, frame, payload = 4096, 8032, 8000
    rng = np.random.default_rng(6)
    buf = rng.integers(0, 256, nframes * frame, dtype=np.uint8)
    got = kernels.count_states(device(buf), nframes, payload, 2, 1, src0=32, src_stride=frame)
    # a second way to the expectation: the histogram of the payload bytes, expanded
    hist = np.bincount(buf.reshape(nframes, frame)[:, 32:].ravel(), minlength=256)
    want = np.zeros(4, np.int64)
    for v in range(256):
        for k in range(4):
            want[(v >> (2 * k)) & 3] += hist[v]
    assert want.sum() == nframes * payload * 4
    assert np.array_equal(got.cpu().numpy().reshape(4), want)
    # two interleaved slots of four positions take every other frame each
    got = kernels.count_states(device(buf), nframes // 2, payload, 2, 4, 2, src0=32, src_stride=frame)
    pay = buf.reshape(nframes // 2, 2, frame)[:, :, 32:]
    for s in range(2):
        hist = np.bincount(pay[:, s].ravel(), minlength=256)
        want = np.zeros((4, 4), np.int64)
        for v in range(256):
            for k in range(4):
                want[k, (v >> (2 * k)) & 3] += hist[v]
        assert np.array_equal(got[s].cpu().numpy(), want)


def test_one_gibibyte_of_zeros_counts_two_to_the_33():
    """The 64-bit total: 2^33 one-bit codes in one bin, more than any 32-bit on-chip
    counter holds -- as 8 KiB frames and as one payload of 1 GiB."""
    from baseband_amd import kernels
    torch = _torch()
    dbuf = torch.zeros(1 << 30, dtype=torch.uint8, device='cuda')
    for nframes, payload in ((1 << 17, 1 << 13), (1, 1 << 30)):
        got = kernels.count_states(dbuf, nframes, payload, 1, 1, src0=0, src_stride=payload)
        assert got.cpu().numpy().reshape(2).tolist() == [2 ** 33, 0]
    del dbuf


def test_argument_errors_leave_the_counts_alone():
    from baseband_amd import _lib, kernels
    torch = _torch()
    bps, chunk, nslot, payload, nframes = 2, 4, 2, 1000, 4
    dbuf = torch.zeros(nframes * nslot * payload, dtype=torch.uint8, device='cuda')
    n = nslot * chunk << bps
    counts = torch.full((n + 1,), 3, dtype=torch.int64, device='cuda')

    def call(ncounts=n, counts_off=0, stride=payload, buf_nbytes=None, dbuf_off=0, **kw):
        p = _lib.StatesParams()
        p.bps, p.chunk, p.nslot, p.payload_nbytes = bps, chunk, nslot, payload
        p.src0, p.src_stride = 0, stride
        p.row_lo, p.row_hi = 0, nframes * (payload * 8 // bps // chunk)
        for k, v in kw.items():
            setattr(p, k, v)
        rc = _lib.lib.bb_count_states(ctypes.c_void_p(dbuf.data_ptr() + dbuf_off),
                                      dbuf.numel() if buf_nbytes is None else buf_nbytes, None, nframes,
                                      ctypes.byref(p), ctypes.c_void_p(counts.data_ptr() + counts_off), ncounts,
                                      kernels._stream(dbuf))
        torch.cuda.synchronize()
        return rc

    assert call(ncounts=n - 1) == _lib.BB_ERANGE
    assert call(stride=payload + 4) == _lib.BB_ERANGE           # the last payload ends outside the buffer
    assert call(buf_nbytes=dbuf.numel() - 1) == _lib.BB_ERANGE
    assert call(counts_off=4) == _lib.BB_EINVAL                 # d_counts not 8-byte aligned
    assert call(dbuf_off=2, buf_nbytes=dbuf.numel() - 2, stride=0) == _lib.BB_EINVAL
    assert call(stride=payload + 2, buf_nbytes=1 << 20) == _lib.BB_EINVAL
    assert call(row_hi=nframes * (payload * 8 // bps // chunk) + 1) == _lib.BB_ERANGE
    assert call(reserved=1) == _lib.BB_EINVAL
    assert call(bps=3) == _lib.BB_ENOTSUP
    assert bool((counts == 3).all())
    with pytest.raises(KeyError):
        kernels.count_states(dbuf, nframes, 1024, 2, 128, 1)
    assert call() == _lib.BB_OK                                 # (the block itself is a good one)
    assert int(counts[:n].sum()) == 3 * n + nframes * nslot * payload * 4 and int(counts[n]) == 3
