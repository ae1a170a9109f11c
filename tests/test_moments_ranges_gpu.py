"""k_i8_moments where one wave walks MANY work items: launches of more than 4096 items, so that every wave
gets a contiguous range of them and carries its partials, its (unit, frame, segment) counter and its fold
counters from item to item.  Every comparison is exact int64; every launch asserts from the bb_last_kernel
note that it has more items than waves and that items and grid are what tests/momentkit.py's `split` says.

  * Ranges that cross everything (RANGE_CASES, random bytes, `momentkit.series_oracle`): ranges that begin
    inside a frame, cross frames, runs and column blocks, hold skipped items (-1, outside the buffer, off a
    dword, a run that ended before its last item) first, last and in the middle, and a last range that is
    short; bins of 7 rows (many per item), of about 1.5 frames (items that share a bin and items that do not)
    and one bin for everything (only the unit change flushes).  The payloads overlap or are named many times,
    so a launch of thousands of frames reads a buffer of about a MiB at the most.
  * The int32 folds (FOLD_CASES, constant bytes at stride 0, closed-form sums): per wave 192 passes of the
    run form (BB_MOM_RUN_FOLD is 64) and 196608 and 131104 rows of the row form (BB_MOM_ROW_FOLD is 65536),
    at -128, 127 and an alternation of both: a wave that did not fold would wrap its int32 partials.

tests/test_momentkit.py (no device) shows that a model kernel which gets one of these things wrong is caught
by a case named there, and that every case crosses what it is listed for."""
import collections
import re

import numpy as np
import pytest

import guardkit
import momentkit as mk
from momentkit import CF, TF, ROWS

pytestmark = pytest.mark.gpu

FIRST_ROW = 12345                       # a multiple of no bin length used here (asserted)

Case = collections.namedtuple('Case', 'name geom nframes inner mode stride forms')
Case.__doc__ = """geom: (layout, npol, nchan, ncomp, ntime); inner: a (t_lo, t_hi) inside the payload, run next to the
whole payload; mode: what the note must name; stride: of the fixed-stride form, bytes; forms: of 'index', 'stride'."""

BOTH = ('index', 'stride')
RANGE_CASES = (
    # 101 items per run: ranges of 2 straddle a run boundary
    Case('run-many-runs', (CF, 2, 65, 2, 96), 101, (3, 91), 'run', 260, BOTH),
    # ... and ranges of 3 of them: a frame that is skipped lies between two that count
    Case('run-runs-of-three', (CF, 2, 65, 2, 96), 127, (3, 91), 'run', 260, BOTH),
    # 5 items per frame, ranges of 6: they begin inside frames and cross frames and runs
    Case('run-segments', (CF, 1, 3, 2, 40000), 1367, (3, 39995), 'run', 12, BOTH),
    # one run, 3 items per frame, ranges of 4; the inner times are 2 items and a third that only payloads
    # off 16 bytes have
    Case('run-one-run', (ROWS, 1, 1, 1, 40000), 4097, (4, 32772), 'run', 4, BOTH),
    Case('run-tf-one-channel', (TF, 2, 1, 2, 20000), 1367, (3, 19995), 'run', 12, BOTH),
    # 3 lane columns (no power of two): 21 rows per wave load, 3 items per frame
    Case('rows4-narrow', (ROWS, 2, 3, 2, 1400), 1401, (3, 1395), 'rows4', 24, BOTH),
    # 65 lane columns: two column blocks of 6147 items, ranges of 4
    Case('rows4-two-blocks', (TF, 2, 65, 2, 96), 2049, (3, 91), 'rows4', 520, BOTH),
    # an item per frame and column block, ranges of 3
    Case('rows4-frames-of-one', (TF, 2, 65, 2, 32), 4099, (3, 27), 'rows4', 260, BOTH),
    # 16 bytes per lane: 17 lane columns, then 2 (a power of two: lanes added by shuffles)
    Case('rows16-nv17', (ROWS, 2, 68, 2, 200), 1401, (3, 198), 'rows16', 544, ('stride',)),
    Case('rows16-nv2', (ROWS, 4, 8, 1, 2100), 1401, (3, 2095), 'rows16', 96, ('stride',)),
)
CASE_FORMS = [(c, f) for c in RANGE_CASES for f in c.forms]
GUARDED = ('run-many-runs', 'rows4-two-blocks')

Fold = collections.namedtuple('Fold', 'name geom nframes buf_align mode')
FOLD_CASES = (
    # per wave 96 items of which 48 hold bytes (the second item of an aligned run is empty): 192 passes
    Fold('run', (ROWS, 1, 1, 1, 16384), 3 << 16, 0, 'run'),
    # 2 lane columns, items of 1024 rows, 192 a wave: 196608 rows
    Fold('rows-shuffled', (ROWS, 2, 2, 2, 1024), 3 << 18, 0, 'rows4'),
    # 64 lane columns (a buffer off 16 bytes keeps the lanes at 4 bytes), items of 32 rows, 4097 a wave: 131104 rows
    Fold('rows-lane-per-column', (ROWS, 2, 64, 2, 32), (1 << 24) + 4096, 4, 'rows4'),
)
FOLD_VALUES = (-128, 127, 'both')
FOLD_BIN = 100003                       # a prime


def _torch():
    import torch
    return torch


def t_ranges(case):
    return ((0, case.geom[4]), case.inner)


def bin_lengths(case, nt):
    return (7, 3 * nt // 2 + 1, FIRST_ROW + case.nframes * nt + 11)


def inputs(case, form, t_lo, t_hi):
    """-> (buf, offsets, wide, launch keywords but for the index)."""
    rng = np.random.default_rng([RANGE_CASES.index(case), BOTH.index(form), t_lo])
    if form == 'index':
        buf, offsets = mk.indexed(case.geom, case.nframes, t_lo, t_hi, rng)
        return buf, offsets, False, {}
    wide = case.mode == 'rows16'
    src0 = 64 if wide or t_lo == 0 else 68
    buf, offsets = mk.strided(case.geom, case.nframes, src0, case.stride, rng)
    return buf, offsets, wide, dict(src0=src0, src_stride=case.stride)


def launch(dbuf, nframes, geom, t_lo, t_hi, bin_rows, nbins, **kw):
    from baseband_amd import kernels
    return kernels.i8_moments(dbuf, nframes, geom[0], geom[1], geom[2], geom[3], geom[4], t_lo, t_hi, bin_rows, nbins, **kw)


def note():
    """-> (mode, grid, items) of the last launch."""
    from baseband_amd import _lib
    m = re.match(r'k_i8_moments<(\w+)> grid (\d+) items (\d+)$', _lib.last_kernel())
    assert m, _lib.last_kernel()
    return m.group(1), int(m.group(2)), int(m.group(3))


def assert_many_items(s, mode):
    got_mode, grid, items = note()
    assert got_mode == mode == s.mode
    assert items > 4 * grid, (items, grid)                      # a wave walks more than one item
    assert (items, grid) == (s.nwork, s.grid), (items, grid, s.nwork, s.grid)


def on_device(buf, align=0):
    """The bytes in device memory, `align` bytes off a multiple of 16."""
    torch = _torch()
    d = torch.empty(buf.size + 16, dtype=torch.uint8, device='cuda')
    assert d.data_ptr() % 16 == 0
    d = d[align:align + buf.size]
    d.copy_(torch.from_numpy(buf))
    return d


@pytest.mark.parametrize('case,form', CASE_FORMS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_ranges_that_cross_everything(case, form):
    torch = _torch()
    layout, npol, nchan, ncomp, ntime = case.geom
    for t_lo, t_hi in t_ranges(case):
        buf, offsets, wide, kw = inputs(case, form, t_lo, t_hi)
        dbuf = on_device(buf)
        if form == 'index':
            kw = dict(src=torch.from_numpy(offsets).cuda())
        s = mk.split(layout, npol, nchan, ncomp, ntime, case.nframes, t_lo, t_hi, wide)
        nt = t_hi - t_lo
        for bin_rows in bin_lengths(case, nt):
            assert FIRST_ROW % bin_rows
            nbins = (FIRST_ROW + case.nframes * nt - 1) // bin_rows + 1
            got = launch(dbuf, case.nframes, case.geom, t_lo, t_hi, bin_rows, nbins, first_row=FIRST_ROW, **kw)
            assert_many_items(s, case.mode)
            want = mk.series_oracle(buf, offsets, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, FIRST_ROW)
            assert want.any()
            assert np.array_equal(got.cpu().numpy(), want), (t_lo, t_hi, bin_rows)
            del got, want


@pytest.mark.parametrize('name', GUARDED)
def test_ranges_add_to_what_the_sums_held_between_guard_words(name):
    """As test_guarded_output_and_untouched_bins of tests/test_moments_kernels_gpu.py, with ranges of items."""
    torch = _torch()
    case = [c for c in RANGE_CASES if c.name == name][0]
    layout, npol, nchan, ncomp, ntime = case.geom
    R = mk.row_bytes(layout, npol, nchan, ncomp)
    t_lo, t_hi = case.inner
    nt = t_hi - t_lo
    buf, offsets, wide, _ = inputs(case, 'index', t_lo, t_hi)
    s = mk.split(layout, npol, nchan, ncomp, ntime, case.nframes, t_lo, t_hi, wide)
    bin_rows = bin_lengths(case, nt)[1]
    nbins = (FIRST_ROW + case.nframes * nt - 1) // bin_rows + 1 + 4      # the bins in front of the first row and 4 behind the last stay
    nelem = nbins * R * 2
    rng = np.random.default_rng(17)
    whole, view = guardkit.poisoned(2 * nelem, torch.int32)
    held = rng.integers(-2 ** 40, 2 ** 40, nelem, dtype=np.int64)
    sums = view.view(torch.int64)
    assert sums.data_ptr() % 8 == 0 and sums.numel() == nelem
    sums.copy_(torch.from_numpy(held).cuda())
    launch(on_device(buf), case.nframes, case.geom, t_lo, t_hi, bin_rows, nbins, first_row=FIRST_ROW,
           src=torch.from_numpy(offsets).cuda(), sums=sums.view(nbins, npol, nchan, ncomp, 2))
    assert_many_items(s, case.mode)
    want = mk.series_oracle(buf, offsets, layout, npol, nchan, ncomp, ntime, t_lo, t_hi, bin_rows, nbins, FIRST_ROW,
                            sums=held.copy().reshape(nbins, npol, nchan, ncomp, 2))
    front = FIRST_ROW // bin_rows
    assert front > 0 and np.array_equal(want[:front].reshape(-1), held[:front * R * 2])
    assert np.array_equal(want[-4:].reshape(-1), held[-4 * R * 2:]) and not np.array_equal(want.reshape(-1), held)
    v = guardkit.verdict(whole, view, want.reshape(-1).view(np.int32))
    assert guardkit.clean(v), (name, guardkit.describe(v, 2 * nelem))


def fold_payload(fold, value):
    """One payload: every byte `value`, or -128 at the even times and 127 at the odd ones ('both': the sum
    nearly cancels, the squares do not)."""
    layout, npol, nchan, ncomp, ntime = fold.geom
    R = mk.row_bytes(layout, npol, nchan, ncomp)
    if value == 'both':
        rows = np.where(np.arange(ntime) % 2 == 0, -128, 127)
    else:
        rows = np.full(ntime, value)
    return np.repeat(rows.astype(np.int8), R).view(np.uint8)


def fold_expected(fold, value, nframes, bin_rows):
    """Sums of x and of x * x per bin of `nframes` such payloads, in Python integers -> int64 (nbins, 2)."""
    ntime = fold.geom[4]
    assert ntime % 2 == 0                                       # the parity of a time is that of its row
    nrows = nframes * ntime
    out = []
    for b in range(-(-nrows // bin_rows)):
        lo, hi = b * bin_rows, min((b + 1) * bin_rows, nrows)
        even = (hi + 1) // 2 - (lo + 1) // 2
        odd = hi - lo - even
        a, c = (-128, 127) if value == 'both' else (value, value)
        out.append((a * even + c * odd, a * a * even + c * c * odd))
    return np.array(out, np.int64)


@pytest.mark.parametrize('value', FOLD_VALUES)
@pytest.mark.parametrize('fold', FOLD_CASES, ids=lambda f: f.name)
def test_int32_partials_are_folded_before_they_wrap(fold, value):
    layout, npol, nchan, ncomp, ntime = fold.geom
    dbuf = on_device(fold_payload(fold, value), fold.buf_align)
    s = mk.split(layout, npol, nchan, ncomp, ntime, fold.nframes, 0, ntime, False)
    nrows = fold.nframes * ntime
    for bin_rows in (nrows, FOLD_BIN):
        want = fold_expected(fold, value, fold.nframes, bin_rows)
        if bin_rows == nrows:
            assert want.shape == (1, 2) and want[0, 1] > 1 << 40   # (far beyond 32 bits: the case has not shrunk)
        got = launch(dbuf, fold.nframes, fold.geom, 0, ntime, bin_rows, len(want), src0=0, src_stride=0)
        assert_many_items(s, fold.mode)
        got = got.cpu().numpy()
        assert got.shape == (len(want), npol, nchan, ncomp, 2)
        assert np.array_equal(got, np.broadcast_to(want[:, None, None, None, :], got.shape)), (fold.name, value, bin_rows)
