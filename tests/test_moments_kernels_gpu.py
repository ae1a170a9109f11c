"""bb_i8_moments (k_i8_moments) against a NumPy int64 oracle written here: every comparison
is exact.  Geometries are the smallest at which the kernel takes another path: one and
several runs, rows narrower and wider than a wave load, rows of 4- and 16-byte lane columns,
payloads on and off 16 bytes, edges inside a dword, bins shorter than a load and longer than
the request."""
import numpy as np
import pytest

import guardkit
import seamkit as sk
from momentkit import CF, TF, ROWS, oracle, row_bytes, samples

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def launch(dbuf, nframes, geom, ntime, t_lo, t_hi, bin_rows, nbins, **kw):
    from baseband_amd import kernels
    return kernels.i8_moments(dbuf, nframes, geom[0], geom[1], geom[2], geom[3], ntime, t_lo, t_hi, bin_rows, nbins, **kw)


def last_kernel():
    from baseband_amd import _lib
    return _lib.last_kernel()


GEOMETRIES = (
    [(CF, npol, nchan, 2, ntime) for npol in (1, 2) for nchan in (1, 3, 64, 65) for ntime in (96, 1000)]
    + [(TF, 2, nchan, 2, 96) for nchan in (1, 8, 65, 4100)] + [(TF, 2, 8, 2, 1000)]
    # rows of R = 1, 2, 4, 8, 12, 260 and 16388 bytes
    + [(ROWS, 1, 1, 1, 1001), (ROWS, 1, 1, 2, 1001), (ROWS, 2, 1, 1, 999), (ROWS, 2, 1, 2, 1001), (ROWS, 1, 2, 2, 96),
       (ROWS, 2, 2, 2, 1000), (ROWS, 2, 3, 2, 1000), (ROWS, 2, 65, 2, 96), (ROWS, 2, 4097, 2, 96), (ROWS, 4, 4, 2, 1000)])


@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: "{}-p{}-c{}-k{}-t{}".format('CF TF ROWS'.split()[g[0]], *g[1:]))
def test_geometries_and_edges(geom):
    """Three frames at a stride with padding between the payloads, on and off 16 bytes; every
    (t_lo, t_hi), bin length and first row."""
    torch = _torch()
    layout, npol, nchan, ncomp, ntime = geom
    R = row_bytes(layout, npol, nchan, ncomp)
    pay = ntime * R
    rng = np.random.default_rng(hash(geom) % 2 ** 32)
    stride = pay + (-pay) % 16 + 48
    for src0 in (64, 68):
        buf = rng.integers(0, 256, src0 + 2 * stride + pay + (-pay) % 4, dtype=np.uint8)
        dbuf = torch.from_numpy(buf).cuda()
        assert dbuf.data_ptr() % 16 == 0
        offsets = [src0 + k * stride for k in range(3)]
        for t_lo, t_hi in ((0, ntime), (3, ntime - 5), (1, 2)):
            nt = t_hi - t_lo
            for bin_rows in (1, 7, 256, 3 * nt + 11):
                for first_row in (0, 5):
                    nbins = (first_row + 3 * nt - 1) // bin_rows + 1
                    got = launch(dbuf, 3, geom, ntime, t_lo, t_hi, bin_rows, nbins, first_row=first_row,
                                 src0=src0, src_stride=stride)
                    assert last_kernel().startswith('k_i8_moments')
                    want = oracle(buf, offsets, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, first_row)
                    assert got.shape == want.shape and got.dtype == torch.int64
                    assert np.array_equal(got.cpu().numpy(), want), (src0, t_lo, t_hi, bin_rows, first_row)
    # the wide loads are taken where every row begins on 16 bytes
    if layout != CF and R > 4 and R % 16 == 0:
        launch(dbuf[4:], 3, geom, ntime, 0, ntime, 7, 3 * ntime, src0=64, src_stride=stride)
        assert 'rows4' in last_kernel()
        launch(torch.from_numpy(buf[4:]).cuda(), 3, geom, ntime, 0, ntime, 7, 3 * ntime, src0=64, src_stride=stride)
        assert 'rows16' in last_kernel()


def test_index_scrambled_with_a_missing_frame_and_a_payload_at_the_buffers_end():
    torch = _torch()
    rng = np.random.default_rng(11)
    for geom in ((CF, 2, 3, 2, 200), (TF, 2, 8, 2, 200), (ROWS, 2, 3, 2, 200), (ROWS, 1, 1, 2, 202)):
        layout, npol, nchan, ncomp, ntime = geom
        pay = ntime * row_bytes(layout, npol, nchan, ncomp)
        stride = pay + 20
        buf = rng.integers(0, 256, 4 * stride + pay, dtype=np.uint8)      # the fifth payload ends the buffer
        dbuf = torch.from_numpy(buf).cuda()
        offsets = np.array([3 * stride, -1, 4 * stride, 0, buf.size - pay + 4, stride, -7, 2 * stride + 2], np.int64)
        src = torch.from_numpy(offsets).cuda()
        nt, bin_rows = ntime - 9, 50
        nbins = -(-len(offsets) * nt // bin_rows)
        got = launch(dbuf, len(offsets), geom, ntime, 4, ntime - 5, bin_rows, nbins, src=src)
        want = oracle(buf, offsets, layout, npol, nchan, ncomp, ntime, 4, ntime - 5, bin_rows, nbins)
        assert np.array_equal(got.cpu().numpy(), want), geom
        # at the fixed stride the last payload ends exactly at the buffer's end; one frame more is refused
        got = launch(dbuf, 5, geom, ntime, 0, ntime, bin_rows, 5 * ntime, src0=0, src_stride=stride)
        want = oracle(buf, [k * stride for k in range(5)], layout, npol, nchan, ncomp, ntime, 0, ntime, bin_rows, 5 * ntime)
        assert np.array_equal(got.cpu().numpy(), want), geom
        from baseband_amd import _lib
        with pytest.raises(_lib.BBError):
            launch(dbuf, 6, geom, ntime, 0, ntime, bin_rows, 6 * ntime, src0=0, src_stride=stride)


def test_two_launches_fill_one_answer():
    torch = _torch()
    rng = np.random.default_rng(12)
    for geom in ((CF, 2, 5, 2, 300), (TF, 2, 8, 2, 300), (ROWS, 2, 1, 2, 300)):
        layout, npol, nchan, ncomp, ntime = geom
        pay = ntime * row_bytes(layout, npol, nchan, ncomp)
        buf = rng.integers(0, 256, 4 * pay, dtype=np.uint8)
        dbuf = torch.from_numpy(buf).cuda()
        nbins = -(-4 * ntime // 64)
        one = launch(dbuf, 4, geom, ntime, 0, ntime, 64, nbins, src0=0, src_stride=pay)
        two = launch(dbuf, 1, geom, ntime, 0, ntime, 64, nbins, src0=0, src_stride=pay)
        # the second frame in two pieces with different row ranges, then the last two
        launch(dbuf, 1, geom, ntime, 0, 101, 64, nbins, first_row=ntime, src0=pay, src_stride=pay, sums=two)
        launch(dbuf, 1, geom, ntime, 101, ntime, 64, nbins, first_row=ntime + 101, src0=pay, src_stride=pay, sums=two)
        launch(dbuf, 2, geom, ntime, 0, ntime, 64, nbins, first_row=2 * ntime, src0=2 * pay, src_stride=pay, sums=two)
        assert torch.equal(one, two)
        assert np.array_equal(one.cpu().numpy(), oracle(buf, [k * pay for k in range(4)], layout, npol, nchan, ncomp,
                                                        ntime, 0, ntime, 64, nbins))


@pytest.mark.parametrize('npol,n,value', [(2, (1 << 17) + 1, -128), (1, (1 << 24) + 1, -128), (1, (1 << 24) + 1, 127)])
def test_sums_wider_than_32_bits(npol, n, value):
    """One run in one bin: the sum of squares passes 2^31 after 2^17 times of -128, the sum
    itself -2^31 after 2^24 (channels first, one channel; an even number of times stored at one
    polarisation, as the pitch must be whole dwords)."""
    torch = _torch()
    ntime = n + (n % 2 if npol == 1 else 0)
    dbuf = torch.full((ntime * npol * 2,), value, dtype=torch.int8, device='cuda').view(torch.uint8)
    got = launch(dbuf, 1, (CF, npol, 1, 2), ntime, 0, n, n, 2)
    want = np.zeros((2, npol, 1, 2, 2), np.int64)
    want[0, ..., 0], want[0, ..., 1] = value * n, value * value * n
    assert abs(value * n) > 1 << 31 or value * value * n > 1 << 31
    assert np.array_equal(got.cpu().numpy(), want)
    # ... and in bins that do not divide a wave load
    got = launch(dbuf, 1, (CF, npol, 1, 2), ntime, 1, n, 100003, -(-(n - 1) // 100003))
    cnt = np.minimum(100003, (n - 1) - 100003 * np.arange(got.shape[0]))
    assert np.array_equal(got.cpu().numpy()[:, 0, 0, 0, :], np.stack([value * cnt, value * value * cnt], -1))


def test_guarded_output_and_untouched_bins():
    """The sums lie between guard words: those keep their poison, and bins no row falls in keep
    what they held."""
    torch = _torch()
    rng = np.random.default_rng(13)
    for geom in ((CF, 2, 65, 2, 1000), (TF, 2, 65, 2, 96), (ROWS, 2, 3, 2, 1000), (ROWS, 1, 1, 1, 1000)):
        layout, npol, nchan, ncomp, ntime = geom
        R = row_bytes(layout, npol, nchan, ncomp)
        pay = ntime * R
        buf = rng.integers(0, 256, 2 * pay + (-2 * pay) % 4, dtype=np.uint8)
        dbuf = torch.from_numpy(buf).cuda()
        bin_rows, first_row = 37, 3 * 37 + 5                                   # bins 0 - 2 and those behind the last stay as they are
        nbins = (first_row + 2 * ntime - 1) // bin_rows + 1 + 4
        nelem = nbins * R * 2
        whole, view = guardkit.poisoned(2 * nelem, torch.int32)
        held = rng.integers(-2 ** 40, 2 ** 40, nelem, dtype=np.int64)
        sums = view.view(torch.int64)
        assert sums.data_ptr() % 8 == 0 and sums.numel() == nelem
        sums.copy_(torch.from_numpy(held).cuda())
        launch(dbuf, 2, geom, ntime, 0, ntime, bin_rows, nbins, first_row=first_row, src0=0, src_stride=pay,
               sums=sums.view(nbins, npol, nchan, ncomp, 2))
        want = oracle(buf, [0, pay], layout, npol, nchan, ncomp, ntime, 0, ntime, bin_rows, nbins, first_row,
                      sums=held.copy().reshape(nbins, npol, nchan, ncomp, 2))
        assert np.array_equal(want[:3].reshape(-1), held[:3 * R * 2]) and np.array_equal(want[-4:].reshape(-1), held[-4 * R * 2:])
        v = guardkit.verdict(whole, view, want.reshape(-1).view(np.int32))
        assert guardkit.clean(v), (geom, guardkit.describe(v, 2 * nelem))


def test_refusals_launch_nothing():
    torch = _torch()
    from baseband_amd import _lib, kernels
    dbuf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    launch(dbuf, 1, (CF, 2, 4, 2), 96, 0, 96, 8, 12)
    mark = last_kernel()
    assert mark.startswith('k_i8_moments')
    sums = torch.zeros((12, 2, 4, 2, 2), dtype=torch.int64, device='cuda')
    for geom, ntime, kw in (((_lib.MOMENTS_MKBF, 2, 4, 2), 256, {}), ((ROWS, 3, 1, 2), 96, {}), ((CF, 3, 4, 2), 96, {}),
                            ((CF, 1, 4, 2), 97, {}), ((CF, 2, 4, 2), 96, dict(src0=2))):
        with pytest.raises(KeyError):                           # BB_ENOTSUP
            launch(dbuf, 1, geom, ntime, 0, ntime, 8, 13, **kw)
        assert not kernels.i8_moments_supported(geom[0], geom[1], geom[2], geom[3], ntime, **kw)
    with pytest.raises(KeyError):                               # a buffer off a dword
        launch(dbuf[1:], 1, (CF, 2, 4, 2), 96, 0, 96, 8, 12, sums=sums)
    for args, kw in (((96, 0, 97, 8, 13), {}), ((96, 0, 96, 0, 12), {}),                    # BB_EINVAL
                     ((96, 0, 96, 8, 11), dict(sums=sums[:11])),                              # BB_ERANGE: the last row's bin
                     ((96, 0, 96, 8, 12), dict(sums=sums[:11])),                              # ... fewer counters than bins
                     ((96, 0, 96, 8, 12), dict(sums=sums, first_row=1)),
                     ((96, 0, 96, 8, 12), dict(sums=sums, src0=1 << 16))):                    # the payload outside the buffer
        with pytest.raises(_lib.BBError):
            launch(dbuf, 1, (CF, 2, 4, 2), *args, **kw)
    assert last_kernel() == mark
    assert int(sums.abs().sum()) == 0
    # nothing asked for: no launch, no error
    launch(dbuf, 0, (CF, 2, 4, 2), 96, 0, 96, 8, 12, sums=sums)
    launch(dbuf, 1, (CF, 2, 4, 2), 96, 7, 7, 8, 12, sums=sums)
    assert last_kernel() == mark


def test_seams_payloads_past_4_gib_and_rows_past_2_32():
    """Payloads around byte 2^31 and 2^32 of a sparse buffer through the index, and a series
    whose rows lie beyond 2^32 with bins so long that their numbers stay small."""
    torch = _torch()
    free, _ = torch.cuda.mem_get_info()
    if free < sk.SIZE + (1 << 30):
        pytest.skip("{:.1f} GiB of device memory free".format(free / 2 ** 30))
    big = torch.empty(sk.SIZE, dtype=torch.uint8, device='cuda')
    assert big.data_ptr() % 16 == 0
    for geom in ((CF, 2, 3, 2, 1000), (TF, 2, 8, 2, 500), (ROWS, 2, 3, 2, 1000), (ROWS, 2, 1, 2, 1001)):
        layout, npol, nchan, ncomp, ntime = geom
        unit = ntime * row_bytes(layout, npol, nchan, ncomp)
        sparse = sk.Sparse(big, unit, sk.places(unit, sk.SIZE, align=4, odd=False), np.random.default_rng(unit))
        assert max(sparse.at) > sk.HIGH and len(sparse.valid()) >= 8
        small, idx = sparse.compact()
        src = torch.from_numpy(sparse.index()).cuda()
        nt = ntime - 8
        first_row, bin_rows = (1 << 32) + 12345, (1 << 31) + 99999
        nbins = (first_row + len(idx) * nt - 1) // bin_rows + 1
        assert nbins == 2 and first_row // bin_rows == 1       # everything in the last bin ...
        got = launch(big, len(idx), geom, ntime, 3, ntime - 5, bin_rows, nbins, first_row=first_row, src=src)
        want = oracle(small, idx, layout, npol, nchan, ncomp, ntime, 3, ntime - 5, bin_rows, nbins, first_row)
        assert np.array_equal(got.cpu().numpy(), want), geom
        # ... and with a bin edge inside the request
        first_row = 2 * bin_rows - 2 * nt - 7
        assert first_row > 1 << 32
        got = launch(big, len(idx), geom, ntime, 3, ntime - 5, bin_rows, 3, first_row=first_row, src=src)
        want = oracle(small, idx, layout, npol, nchan, ncomp, ntime, 3, ntime - 5, bin_rows, 3, first_row)
        assert np.array_equal(got.cpu().numpy(), want), geom
        assert want[1].any() and want[2].any() and not want[0].any()
        # at the fixed stride from a first payload behind the high seam
        off = sk.HIGH + 4096 + 4
        st = sk.Strided(big, off, unit + 52, 3, unit, np.random.default_rng(unit + 1))
        small, idx = st.compact()
        got = launch(big, 3, geom, ntime, 0, ntime, 100, 3 * ntime, src0=off, src_stride=unit + 52)
        want = oracle(small, idx, layout, npol, nchan, ncomp, ntime, 0, ntime, 100, 3 * ntime)
        assert np.array_equal(got.cpu().numpy(), want), geom
