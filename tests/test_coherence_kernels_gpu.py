"""bb_i8_coherence (k_i8_coherence) against the NumPy int64 oracle of tests/coherencekit.py: every
comparison is exact.  Geometries are the smallest at which the kernel takes another path: one and
several runs, runs under one wave load and of two work items, rows narrower and wider than a wave
load, lane columns of 4 and 16 bytes, X halves of one dword, off 16 bytes and of two column blocks,
payloads on and off 16 bytes, bins shorter than a load and longer than the request."""
import collections
import re

import numpy as np
import pytest

import coherencekit as ck
import guardkit
import momentkit as mk
import seamkit as sk
from coherencekit import CF, TF, ROWS, oracle

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def launch(dbuf, nframes, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, **kw):
    from baseband_amd import kernels
    return kernels.i8_coherence(dbuf, nframes, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, **kw)


def last_kernel():
    from baseband_amd import _lib
    return _lib.last_kernel()


def note():
    """-> (shape, grid, items) of the last launch."""
    m = re.match(r'k_i8_coherence<(\w+)> grid (\d+) items (\d+)$', last_kernel())
    assert m, last_kernel()
    return m.group(1), int(m.group(2)), int(m.group(3))


def on_device(buf, align=0):
    """The bytes in device memory, `align` bytes off a multiple of 16."""
    torch = _torch()
    d = torch.empty(buf.size + 16, dtype=torch.uint8, device='cuda')
    assert d.data_ptr() % 16 == 0
    d = d[align:align + buf.size]
    d.copy_(torch.from_numpy(buf))
    return d


GEOMETRIES = (
    # runs of 96 times (under one wave load), 1000, and 4200 (two work items a run)
    [(CF, nchan, ntime) for nchan in (1, 3, 65) for ntime in (96, 1000, 4200)]
    + [(TF, nchan, 96) for nchan in (1, 8, 65, 4100)] + [(TF, 8, 1000)]
    # X halves of 4, 8, 12, 16, 132, 144 and 260 bytes; nchan 1 is a run
    + [(ROWS, 1, 1001), (ROWS, 2, 1000), (ROWS, 4, 1000), (ROWS, 6, 1000), (ROWS, 8, 1000), (ROWS, 66, 96), (ROWS, 72, 96),
       (ROWS, 130, 96)])


def expected_shape(layout, nchan, wide):
    if nchan == 1 or layout == CF:
        return 'run'
    if layout == TF:
        return 'rows16' if wide and nchan % 4 == 0 else 'rows4'
    return 'split16' if wide and nchan % 8 == 0 else 'split4'


@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: "{}-c{}-t{}".format('CF TF ROWS'.split()[g[0]], *g[1:]))
def test_geometries_and_edges(geom):
    """Three frames at a stride with padding between the payloads, on and off 16 bytes; every
    (t_lo, t_hi), bin length and first row."""
    torch = _torch()
    layout, nchan, ntime = geom
    pay = ntime * 4 * nchan
    rng = np.random.default_rng([layout, nchan, ntime])
    stride = pay + (-pay) % 16 + 48
    for src0 in (64, 68):
        buf = rng.integers(0, 256, src0 + 2 * stride + pay, dtype=np.uint8)
        buf[src0:src0 + 8] = np.array(ck.EXTREME, np.int8).reshape(-1).view(np.uint8)
        dbuf = torch.from_numpy(buf).cuda()
        assert dbuf.data_ptr() % 16 == 0
        offsets = [src0 + k * stride for k in range(3)]
        for t_lo, t_hi in ((0, ntime), (3, ntime - 5), (1, 2)):
            nt = t_hi - t_lo
            s = ck.split(layout, nchan, ntime, 3, t_lo, t_hi, src0 % 16 == 0)
            for bin_rows in (1, 7, 256, 3 * nt + 11):
                for first_row in (0, 5):
                    nbins = (first_row + 3 * nt - 1) // bin_rows + 1
                    got = launch(dbuf, 3, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, first_row=first_row,
                                 src0=src0, src_stride=stride)
                    assert note() == (expected_shape(layout, nchan, src0 % 16 == 0), s.grid, s.nwork) and s.mode == note()[0]
                    want = oracle(buf, offsets, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, first_row)
                    assert got.shape == want.shape == (nbins, nchan, 4) and got.dtype == torch.int64
                    assert np.array_equal(got.cpu().numpy(), want), (src0, t_lo, t_hi, bin_rows, first_row)


def test_the_note_names_the_shape():
    """rows16 and split16 only where every row begins on 16 bytes: the buffer, the first offset, the stride,
    the row (the X half), and no index."""
    torch = _torch()
    buf = np.random.default_rng(5).integers(0, 256, 1 << 16, dtype=np.uint8)
    whole = on_device(buf, 0)
    off4 = on_device(buf, 4)
    src = torch.tensor([64, 64 + 8192], dtype=torch.int64, device='cuda')
    for layout, nchan, narrow, wide in ((TF, 8, 'rows4', 'rows16'), (ROWS, 8, 'split4', 'split16'), (ROWS, 16, 'split4', 'split16'),
                                        (TF, 6, 'rows4', 'rows4'), (ROWS, 4, 'split4', 'split4'), (ROWS, 12, 'split4', 'split4'),
                                        (CF, 8, 'run', 'run'), (TF, 1, 'run', 'run'), (ROWS, 1, 'run', 'run')):
        ntime = 100
        want = oracle(buf, [64, 64 + 8192], layout, nchan, ntime, 0, ntime, 7, 30)
        for dbuf, kw, shape, b in ((whole, dict(src0=64, src_stride=8192), wide, buf), (whole, dict(src0=68, src_stride=8192), narrow, None),
                                   (whole, dict(src0=64, src_stride=8200), narrow, None), (whole, dict(src=src), narrow, buf),
                                   (off4, dict(src0=64, src_stride=8192), narrow, buf)):
            got = launch(dbuf, 2, layout, nchan, ntime, 0, ntime, 7, 30, **kw)
            assert note()[0] == shape, (layout, nchan, kw)
            if b is not None:
                assert np.array_equal(got.cpu().numpy(), want), (layout, nchan, kw)


def test_index_scrambled_with_a_missing_frame_and_a_payload_at_the_buffers_end():
    torch = _torch()
    rng = np.random.default_rng(11)
    for layout, nchan, ntime in ((CF, 3, 200), (TF, 8, 200), (ROWS, 6, 200), (ROWS, 8, 200), (ROWS, 1, 202)):
        pay = ntime * 4 * nchan
        stride = pay + 20
        buf = rng.integers(0, 256, 4 * stride + pay, dtype=np.uint8)      # the fifth payload ends the buffer
        dbuf = torch.from_numpy(buf).cuda()
        offsets = np.array([3 * stride, -1, 4 * stride, 0, buf.size - pay + 4, stride, -7, 2 * stride + 2], np.int64)
        src = torch.from_numpy(offsets).cuda()
        nt, bin_rows = ntime - 9, 50
        nbins = -(-len(offsets) * nt // bin_rows)
        got = launch(dbuf, len(offsets), layout, nchan, ntime, 4, ntime - 5, bin_rows, nbins, src=src)
        want = oracle(buf, offsets, layout, nchan, ntime, 4, ntime - 5, bin_rows, nbins)
        assert np.array_equal(got.cpu().numpy(), want), (layout, nchan)
        # at the fixed stride the last payload ends exactly at the buffer's end; one frame more is refused
        got = launch(dbuf, 5, layout, nchan, ntime, 0, ntime, bin_rows, 5 * ntime, src0=0, src_stride=stride)
        want = oracle(buf, [k * stride for k in range(5)], layout, nchan, ntime, 0, ntime, bin_rows, 5 * ntime)
        assert np.array_equal(got.cpu().numpy(), want), (layout, nchan)
        from baseband_amd import _lib
        with pytest.raises(_lib.BBError):
            launch(dbuf, 6, layout, nchan, ntime, 0, ntime, bin_rows, 6 * ntime, src0=0, src_stride=stride)


def test_two_launches_fill_one_answer():
    torch = _torch()
    rng = np.random.default_rng(12)
    for layout, nchan, ntime in ((CF, 5, 300), (TF, 8, 300), (ROWS, 1, 300), (ROWS, 6, 300)):
        pay = ntime * 4 * nchan
        buf = rng.integers(0, 256, 4 * pay, dtype=np.uint8)
        dbuf = torch.from_numpy(buf).cuda()
        nbins = -(-4 * ntime // 64)
        one = launch(dbuf, 4, layout, nchan, ntime, 0, ntime, 64, nbins, src0=0, src_stride=pay)
        two = launch(dbuf, 1, layout, nchan, ntime, 0, ntime, 64, nbins, src0=0, src_stride=pay)
        # the second frame in two pieces with different row ranges, then the last two
        launch(dbuf, 1, layout, nchan, ntime, 0, 101, 64, nbins, first_row=ntime, src0=pay, src_stride=pay, sums=two)
        launch(dbuf, 1, layout, nchan, ntime, 101, ntime, 64, nbins, first_row=ntime + 101, src0=pay, src_stride=pay, sums=two)
        launch(dbuf, 2, layout, nchan, ntime, 0, ntime, 64, nbins, first_row=2 * ntime, src0=2 * pay, src_stride=pay, sums=two)
        assert torch.equal(one, two)
        assert np.array_equal(one.cpu().numpy(), oracle(buf, [k * pay for k in range(4)], layout, nchan, ntime, 0, ntime, 64, nbins))


@pytest.mark.parametrize('which', (0, 1))
@pytest.mark.parametrize('layout,nchan', ((CF, 1), (TF, 2), (ROWS, 2)), ids=('run', 'rows', 'split'))
def test_sums_wider_than_32_bits(layout, nchan, which):
    """The extreme quads as constant input, 2^17 + 1 times in one bin: |X|^2, |Y|^2 and Im pass 2^31 in
    magnitude (Re = 128 a sample stays small), with both signs of Im."""
    torch = _torch()
    n = (1 << 17) + 1
    dbuf = torch.from_numpy(ck.constant_payload(layout, nchan, n, ck.EXTREME[which])).cuda()
    per = ck.EXTREME_SUMS[which]
    assert all(abs(per[k]) * n > 1 << 31 for k in (0, 1, 3)) and (per[3] > 0) == (which == 0)
    got = launch(dbuf, 1, layout, nchan, n, 0, n, n, 2).cpu().numpy()
    want = ck.constant_expected(per, n, n)
    assert got.shape == (2, nchan, 4) and not got[1].any()
    assert np.array_equal(got[:1], np.broadcast_to(want[:, None, :], (1, nchan, 4)))
    # ... and in bins that do not divide a wave load
    want = ck.constant_expected(per, n - 1, 100003)
    got = launch(dbuf, 1, layout, nchan, n, 1, n, 100003, len(want)).cpu().numpy()
    assert np.array_equal(got, np.broadcast_to(want[:, None, :], got.shape))


def test_guarded_output_and_untouched_bins():
    """The sums lie between guard words: those keep their poison, and bins no row falls in keep
    what they held."""
    torch = _torch()
    rng = np.random.default_rng(13)
    for layout, nchan, ntime in ((CF, 65, 1000), (TF, 65, 96), (ROWS, 6, 1000), (ROWS, 130, 96), (ROWS, 1, 1000)):
        pay = ntime * 4 * nchan
        buf = rng.integers(0, 256, 2 * pay, dtype=np.uint8)
        dbuf = torch.from_numpy(buf).cuda()
        bin_rows, first_row = 37, 3 * 37 + 5                                   # bins 0 - 2 and those behind the last stay as they are
        nbins = (first_row + 2 * ntime - 1) // bin_rows + 1 + 4
        nelem = nbins * nchan * 4
        whole, view = guardkit.poisoned(2 * nelem, torch.int32)
        held = rng.integers(-2 ** 40, 2 ** 40, nelem, dtype=np.int64)
        sums = view.view(torch.int64)
        assert sums.data_ptr() % 8 == 0 and sums.numel() == nelem
        sums.copy_(torch.from_numpy(held).cuda())
        launch(dbuf, 2, layout, nchan, ntime, 0, ntime, bin_rows, nbins, first_row=first_row, src0=0, src_stride=pay,
               sums=sums.view(nbins, nchan, 4))
        want = oracle(buf, [0, pay], layout, nchan, ntime, 0, ntime, bin_rows, nbins, first_row,
                      sums=held.copy().reshape(nbins, nchan, 4))
        assert np.array_equal(want[:3].reshape(-1), held[:3 * nchan * 4]) and np.array_equal(want[-4:].reshape(-1), held[-4 * nchan * 4:])
        v = guardkit.verdict(whole, view, want.reshape(-1).view(np.int32))
        assert guardkit.clean(v), ((layout, nchan), guardkit.describe(v, 2 * nelem))


def test_refusals_launch_nothing():
    torch = _torch()
    from baseband_amd import _lib, kernels
    dbuf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    launch(dbuf, 1, CF, 4, 96, 0, 96, 8, 12)
    mark = last_kernel()
    assert mark.startswith('k_i8_coherence<run>')
    sums = torch.zeros((12, 4, 4), dtype=torch.int64, device='cuda')
    # plain rows with an odd number of channels: the Y half begins inside a dword
    for layout, nchan, ntime, kw in ((ROWS, 3, 96, {}), (ROWS, 65, 96, {}), (_lib.MOMENTS_MKBF, 4, 256, {}), (CF, 4, 96, dict(src0=2))):
        with pytest.raises(KeyError):                           # BB_ENOTSUP
            launch(dbuf, 1, layout, nchan, ntime, 0, ntime, 8, 13, **kw)
        assert not kernels.i8_coherence_supported(layout, nchan, ntime, **kw)
        assert last_kernel() == mark
    with pytest.raises(KeyError):                               # a buffer off a dword
        launch(dbuf[1:], 1, CF, 4, 96, 0, 96, 8, 12, sums=sums)
    for args, kw in (((96, 0, 97, 8, 13), {}), ((96, 0, 96, 0, 12), {}),                    # BB_EINVAL
                     ((96, 0, 96, 8, 11), dict(sums=sums[:11])),                              # BB_ERANGE: the last row's bin
                     ((96, 0, 96, 8, 12), dict(sums=sums[:11])),                              # ... fewer sums than bins
                     ((96, 0, 96, 8, 12), dict(sums=sums, first_row=1)),
                     ((96, 0, 96, 8, 12), dict(sums=sums, src0=1 << 16))):                    # the payload outside the buffer
        with pytest.raises(_lib.BBError):
            launch(dbuf, 1, CF, 4, *args, **kw)
    assert last_kernel() == mark
    assert int(sums.abs().sum()) == 0
    # nothing asked for: no launch, no error
    launch(dbuf, 0, CF, 4, 96, 0, 96, 8, 12, sums=sums)
    launch(dbuf, 1, CF, 4, 96, 7, 7, 8, 12, sums=sums)
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
    for layout, nchan, ntime in ((CF, 3, 1000), (TF, 8, 500), (ROWS, 6, 1000), (ROWS, 1, 1001)):
        unit = ntime * 4 * nchan
        sparse = sk.Sparse(big, unit, sk.places(unit, sk.SIZE, align=4, odd=False), np.random.default_rng(unit))
        assert max(sparse.at) > sk.HIGH and len(sparse.valid()) >= 8
        small, idx = sparse.compact()
        src = torch.from_numpy(sparse.index()).cuda()
        nt = ntime - 8
        first_row, bin_rows = (1 << 32) + 12345, (1 << 31) + 99999
        nbins = (first_row + len(idx) * nt - 1) // bin_rows + 1
        assert nbins == 2 and first_row // bin_rows == 1       # everything in the last bin ...
        got = launch(big, len(idx), layout, nchan, ntime, 3, ntime - 5, bin_rows, nbins, first_row=first_row, src=src)
        want = oracle(small, idx, layout, nchan, ntime, 3, ntime - 5, bin_rows, nbins, first_row)
        assert np.array_equal(got.cpu().numpy(), want), (layout, nchan)
        # ... and with a bin edge inside the request
        first_row = 2 * bin_rows - 2 * nt - 7
        assert first_row > 1 << 32
        got = launch(big, len(idx), layout, nchan, ntime, 3, ntime - 5, bin_rows, 3, first_row=first_row, src=src)
        want = oracle(small, idx, layout, nchan, ntime, 3, ntime - 5, bin_rows, 3, first_row)
        assert np.array_equal(got.cpu().numpy(), want), (layout, nchan)
        assert want[1].any() and want[2].any() and not want[0].any()
        # at the fixed stride from a first payload behind the high seam
        off = sk.HIGH + 4096 + 4
        st = sk.Strided(big, off, unit + 52, 3, unit, np.random.default_rng(unit + 1))
        small, idx = st.compact()
        got = launch(big, 3, layout, nchan, ntime, 0, ntime, 100, 3 * ntime, src0=off, src_stride=unit + 52)
        want = oracle(small, idx, layout, nchan, ntime, 0, ntime, 100, 3 * ntime)
        assert np.array_equal(got.cpu().numpy(), want), (layout, nchan)


# ---- ranges: so many frames (overlapping payloads of a small buffer) that a wave walks several items, across frames,
#      runs and column blocks, with frames missing from the index ----
Range = collections.namedtuple('Range', 'name layout nchan ntime nframes stride mode units')
RANGE_CASES = (
    Range('run-many-runs', CF, 65, 100, 201, 48, 'run', 65),
    Range('run-segments', CF, 3, 9000, 501, 16, 'run', 3),              # three items a (run, frame)
    Range('rows4-three-blocks', TF, 130, 80, 801, 520, 'rows4', 3),     # three items a (column block, frame)
    Range('rows16-nv2', TF, 8, 50, 4203, 32, 'rows16', 1),
    Range('split4-two-blocks', ROWS, 130, 80, 1101, 520, 'split4', 2),
    Range('split16-nv3', ROWS, 24, 30, 4203, 96, 'split16', 1),         # three lane columns: no power of two
)


@pytest.mark.parametrize('form', ('stride', 'index'))
@pytest.mark.parametrize('case', RANGE_CASES, ids=lambda c: c.name)
def test_ranges_of_many_items(case, form):
    """The whole payload through an index with missing frames, an inner row range at the fixed stride."""
    torch = _torch()
    layout, nchan, ntime, nframes = case.layout, case.nchan, case.ntime, case.nframes
    pay = ntime * 4 * nchan
    rng = np.random.default_rng([RANGE_CASES.index(case), form == 'index'])
    buf = rng.integers(0, 256, 64 + (nframes - 1) * case.stride + pay, dtype=np.uint8)
    offsets = 64 + case.stride * np.arange(nframes, dtype=np.int64)
    dbuf = on_device(buf)
    if form == 'index':
        rng.shuffle(offsets)
        stray = rng.random(nframes) < 0.05
        offsets[stray] = rng.choice(np.array([-1, buf.size - pay + 4, 66, buf.size + 64]), int(stray.sum()))
        offsets[[0, -1]] = 64, buf.size - pay                   # (a payload that ends the buffer)
        kw, (t_lo, t_hi) = dict(src=torch.from_numpy(offsets).cuda()), (0, ntime)
    else:
        kw, (t_lo, t_hi) = dict(src0=64, src_stride=case.stride), (3, ntime - 5)
    nt = t_hi - t_lo
    s = ck.split(layout, nchan, ntime, nframes, t_lo, t_hi, form == 'stride')
    assert s.mode == (case.mode if form == 'stride' else case.mode.replace('16', '4'))
    assert s.nwork > 4 * s.grid and s.per >= 2 and (form == 'index' or s.units == case.units)
    assert s.units == 1 or (nframes * s.nseg) % s.per                 # a range holds the end of one unit and the start of the next
    for bin_rows in (7, 3 * nt // 2 + 1, 5 + nframes * nt):       # the last: one bin, so a unit change alone must flush
        nbins = (5 + nframes * nt - 1) // bin_rows + 1
        got = launch(dbuf, nframes, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, first_row=5, **kw)
        shape, grid, items = note()
        assert (shape, grid, items) == (s.mode, s.grid, s.nwork) and items > 4 * grid
        want = oracle(buf, offsets, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, 5)
        assert want.any() and np.array_equal(got.cpu().numpy(), want), (t_lo, t_hi, bin_rows)


# ---- the folds: constant quads at stride 0 over so many frames that a wave walks many items; without its fold an
#      int32 partial of every wave would pass 2^31 (tests/test_coherencekit.py does the sums) ----
Fold = collections.namedtuple('Fold', 'name layout nchan ntime nframes mode')
FOLD_CASES = (
    # per wave 48 items of which 24 hold bytes (the second item of an aligned run is empty): 96 passes
    Fold('run', CF, 1, mk.RUN_STEPS * mk.STEP // 4, 3 * ck.RUN_FOLD // (mk.RUN_STEPS // mk.U) * mk.GRID_WAVES, 'run'),
    # 2 lane columns, items of 1024 rows, 96 a wave: 98304 rows
    Fold('rows', TF, 2, 32 * mk.ROW_STEPS, 3 * ck.ROW_FOLD // (32 * mk.ROW_STEPS) * mk.GRID_WAVES, 'rows4'),
    Fold('split', ROWS, 4, 32 * mk.ROW_STEPS, 3 * ck.ROW_FOLD // (32 * mk.ROW_STEPS) * mk.GRID_WAVES, 'split4'),
)
FOLD_BIN = 100003                       # a prime


@pytest.mark.parametrize('which', (0, 1))
@pytest.mark.parametrize('fold', FOLD_CASES, ids=lambda f: f.name)
def test_int32_partials_are_folded_before_they_wrap(fold, which):
    dbuf = on_device(ck.constant_payload(fold.layout, fold.nchan, fold.ntime, ck.EXTREME[which]))
    assert dbuf.numel() <= 1 << 20
    s = ck.split(fold.layout, fold.nchan, fold.ntime, fold.nframes, 0, fold.ntime, True)
    nrows = fold.nframes * fold.ntime
    for bin_rows in (nrows, FOLD_BIN):
        want = ck.constant_expected(ck.EXTREME_SUMS[which], nrows, bin_rows)
        if bin_rows == nrows:
            assert want.shape == (1, 4) and want[0, 0] > 1 << 40    # (far beyond 32 bits: the case has not shrunk)
        got = launch(dbuf, fold.nframes, fold.layout, fold.nchan, fold.ntime, 0, fold.ntime, bin_rows, len(want), src0=0, src_stride=0)
        shape, grid, items = note()
        assert shape == fold.mode == s.mode and items > 4 * grid and (items, grid) == (s.nwork, s.grid)
        got = got.cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(want[:, None, :], got.shape)), (fold.name, which, bin_rows)
