"""tests/momentkit.py and the case lists of tests/test_moments_ranges_gpu.py, without a device: the split is the
host's, every case crosses what it is listed for, `series_oracle` is the plain `oracle`, the faultless model
kernel equals the oracle on every case, and each fault that the model can be told to make -- a counter that
stops at a skipped item, no flush at a unit change, a bin carried on from a range's first item, a short last
range dropped, no fold, a fold 8 times too late -- is caught by the cases named here."""
import os
import re

import numpy as np
import pytest

import momentkit as mk
import test_moments_ranges_gpu as rg
from momentkit import CF, ROWS

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, 'baseband_amd', 'csrc')

# (items, items of a range, items per (unit, frame), units) at the whole payload, as the note and `split` must give them
NUMBERS = {
    'run-many-runs': (6565, 2, 1, 65), 'run-segments': (20505, 6, 5, 3), 'run-one-run': (12291, 4, 3, 1),
    'run-tf-one-channel': (6835, 2, 5, 1), 'rows4-narrow': (4203, 2, 3, 1), 'rows4-two-blocks': (12294, 4, 3, 2),
    'rows16-nv17': (4203, 2, 3, 1), 'rows16-nv2': (4203, 2, 3, 1),
    'run-runs-of-three': (8255, 3, 1, 65), 'rows4-frames-of-one': (8198, 3, 1, 2),
}
SKIPPED_BETWEEN = ('run-runs-of-three', 'rows4-frames-of-one')     # ranges longer than a frame's items by 2 or more


def _defines(name):
    with open(os.path.join(CSRC, name)) as f:
        return dict(re.findall(r'^#define\s+(\w+)\s+(\d+)', f.read(), re.M))


def test_the_constants_are_the_sources():
    d = _defines('k_moments.h')
    got = [int(d[k]) for k in ('BB_MOM_U', 'BB_MOM_STEP', 'BB_MOM_RUN_STEPS', 'BB_MOM_ROW_STEPS', 'BB_MOM_RUN_FOLD', 'BB_MOM_ROW_FOLD')]
    assert got == [mk.U, mk.STEP, mk.RUN_STEPS, mk.ROW_STEPS, mk.RUN_FOLD, mk.ROW_FOLD]
    c = _defines('bb_common.h')
    assert int(c['BB_WAVE']) == mk.WAVE and int(c['BB_BLOCK']) == mk.WAVE * mk.WAVES_PER_BLOCK
    assert int(_defines('bb_packed.inc')['BB_MOMENTS_GRID']) * mk.WAVES_PER_BLOCK == mk.GRID_WAVES


def test_split_of_small_launches():
    """What tests/test_moments_kernels_gpu.py launches: an item per wave."""
    s = mk.split(CF, 2, 65, 2, 1000, 3, 0, 1000, False)
    assert (s.mode, s.nseg, s.units, s.nwork, s.per, s.ranges, s.grid) == ('run', 1, 65, 195, 1, 195, 49)
    assert s.item(194) == (64, 2, 0) and s.range_of(194) == (194, 195)
    s = mk.split(ROWS, 2, 4097, 2, 96, 3, 0, 96, True)          # rows of 16388 bytes: no multiple of 16
    assert (s.mode, s.NV, s.rpl, s.chunk_rows, s.nseg, s.units, s.nwork) == ('rows4', 4097, 1, 32, 3, 65, 585)
    s = mk.split(ROWS, 4, 4, 2, 1000, 3, 0, 1000, True)
    assert (s.mode, s.NV, s.rpl, s.chunk_rows, s.nseg, s.units, s.nwork) == ('rows16', 2, 32, 1024, 1, 1, 3)
    s = mk.split(CF, 2, 1, 2, (1 << 17) + 1, 1, 0, (1 << 17) + 1, False)
    assert (s.nwork, s.per) == (33, 1)                          # test_sums_wider_than_32_bits: 4 passes an item


@pytest.mark.parametrize('case', rg.RANGE_CASES, ids=lambda c: c.name)
def test_every_case_crosses_what_it_is_listed_for(case):
    assert rg.FIRST_ROW > 0
    for form in case.forms:
        for t_lo, t_hi in rg.t_ranges(case):
            buf, offsets, wide, kw = rg.inputs(case, form, t_lo, t_hi)
            assert buf.size < 1 << 21 and len(offsets) == case.nframes
            s = mk.split(*case.geom, case.nframes, t_lo, t_hi, wide)
            items, per, nseg, units = NUMBERS[case.name]
            assert (s.per, s.nseg, s.units, s.mode) == (per, nseg, units, case.mode), (form, t_lo)
            if (t_lo, t_hi) == (0, case.geom[4]):
                assert s.nwork == items
            assert s.nwork > 4 * s.grid and s.per > 1
            x = mk.crossings(s, offsets, buf.size)
            assert x['frame'] and x['short'] and x['mid_frame'] == (nseg > 1) and x['unit'] == (units > 1), (form, t_lo, x)
            assert all(rg.FIRST_ROW % b for b in rg.bin_lengths(case, t_hi - t_lo))
            if form == 'index':
                # the skipped items: every kind is there, and some are the first, some the last, some inside a range
                assert x['skip_then_count'] and x['count_skip_count'] == (case.name in SKIPPED_BETWEEN)
                assert not wide and not kw
                ok = mk.valid_sources(offsets, buf.size, case.geom[4] * mk.row_bytes(*case.geom[:4]))
                assert 0.99 > ok.mean() > 0.5 and (offsets == -1).any() and (offsets > buf.size).any()
                assert (offsets % 4 == 2).any()
                pay = case.geom[4] * mk.row_bytes(*case.geom[:4])
                assert (offsets == buf.size - pay).any() and (offsets == buf.size - pay + 4).any()
                skip = mk.skipped_items(s, offsets, buf.size)
                w = np.flatnonzero(skip)
                at = w % s.per
                assert (at == 0).sum() >= 3 and (at == s.per - 1).sum() >= 3
                if s.per > 2:
                    assert ((at > 0) & (at < s.per - 1)).sum() >= 3
            else:
                assert kw['src_stride'] % 4 == 0 and kw['src_stride'] <= 3 * max(4, mk.row_bytes(*case.geom[:4]))
                assert wide == (case.mode == 'rows16') and (not wide or (kw['src0'] | kw['src_stride']) % 16 == 0)
                assert offsets[-1] + case.geom[4] * mk.row_bytes(*case.geom[:4]) == buf.size
    if case.name == 'run-one-run':
        # runs that end before their last item: at the stride, where no source is missing, some do and some do not
        buf, offsets, wide, kw = rg.inputs(case, 'stride', *case.inner)
        skip = mk.skipped_items(mk.split(*case.geom, case.nframes, *case.inner, wide), offsets, buf.size)
        assert 0.1 < skip.reshape(-1, 3)[:, 2].mean() < 0.5 and not skip.reshape(-1, 3)[:, :2].any()


@pytest.mark.parametrize('case', rg.RANGE_CASES, ids=lambda c: c.name)
def test_series_oracle_is_the_plain_oracle(case):
    """On the first 48 frames of every input, every row range and bin length."""
    for form in case.forms:
        for t_lo, t_hi in rg.t_ranges(case):
            buf, offsets, _, _ = rg.inputs(case, form, t_lo, t_hi)
            offsets = offsets[:48]
            nt = t_hi - t_lo
            for bin_rows in (7, 3 * nt // 2 + 1, rg.FIRST_ROW + 48 * nt + 11):
                nbins = (rg.FIRST_ROW + 48 * nt - 1) // bin_rows + 1
                a = mk.oracle(buf, offsets, *case.geom, t_lo, t_hi, bin_rows, nbins, rg.FIRST_ROW)
                b = mk.series_oracle(buf, offsets, *case.geom, t_lo, t_hi, bin_rows, nbins, rg.FIRST_ROW, chunk=50000)
                assert a.any() and np.array_equal(a, b), (form, t_lo, bin_rows)


def _verdict(case, form, which_t, which_bin, fault=None):
    """Does the model kernel, with `fault`, give the oracle's sums on one launch of a case?"""
    t_lo, t_hi = rg.t_ranges(case)[which_t]
    buf, offsets, wide, _ = rg.inputs(case, form, t_lo, t_hi)
    nt = t_hi - t_lo
    bin_rows = rg.bin_lengths(case, nt)[which_bin]
    nbins = (rg.FIRST_ROW + case.nframes * nt - 1) // bin_rows + 1
    got = mk.model(buf, offsets, *case.geom, t_lo, t_hi, bin_rows, nbins, rg.FIRST_ROW, wide=wide, fault=fault)
    np.negative(got, out=got)
    mk.series_oracle(buf, offsets, *case.geom, t_lo, t_hi, bin_rows, nbins, rg.FIRST_ROW, sums=got)
    return not got.any()


@pytest.mark.parametrize('case,form', rg.CASE_FORMS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_the_faultless_model_is_the_oracle(case, form):
    for which_t in (0, 1):
        for which_bin in (0, 1, 2):
            if which_bin == 0 and which_t != rg.BOTH.index(form):
                continue                                        # (bins of 7 rows are millions of bins: once per input form)
            assert _verdict(case, form, which_t, which_bin), (which_t, which_bin)


# fault -> launches that catch it: (case, form, row range (0: whole, 1: inner), bin length (0: 7 rows, 1: 1.5 frames, 2: one bin))
CAUGHT_BY = {
    'stuck_counter': [('run-many-runs', 'index', 0, 2), ('run-segments', 'index', 1, 1), ('rows4-narrow', 'index', 0, 1),
                      ('run-one-run', 'stride', 1, 1)],         # (the last: runs that ended, no source missing)
    'no_unit_flush': [('run-many-runs', 'stride', 0, 2), ('run-runs-of-three', 'index', 1, 2), ('run-segments', 'stride', 0, 2), ('rows4-two-blocks', 'stride', 1, 2)],
    # (a unit change takes the series back to its start: the stride form; a skipped frame between two counted ones)
    'first_bin': [('run-many-runs', 'stride', 0, 1), ('rows4-two-blocks', 'stride', 0, 1), ('run-runs-of-three', 'index', 0, 0),
                  ('rows4-frames-of-one', 'index', 1, 1)],
    'drop_last': [(c.name, c.forms[-1], 0, 1) for c in rg.RANGE_CASES],
}


@pytest.mark.parametrize('fault', sorted(CAUGHT_BY))
def test_every_walk_fault_is_caught_by_named_cases(fault):
    by_name = {c.name: c for c in rg.RANGE_CASES}
    for name, form, which_t, which_bin in CAUGHT_BY[fault]:
        assert not _verdict(by_name[name], form, which_t, which_bin, fault), (fault, name, form)


def test_the_fault_list_is_covered():
    assert set(CAUGHT_BY) | {'no_fold', 'fold_x8'} == set(mk.FAULTS)
    assert set(rg.GUARDED) <= set(NUMBERS) and set(NUMBERS) == set(c.name for c in rg.RANGE_CASES)


# ---- the folds.  The model walks 8 waves of the launch, not 4096: as many frames fewer, the same range per wave. ----
WAVES = 8


def _scaled(fold):
    assert fold.nframes * WAVES % mk.GRID_WAVES == 0
    return fold.nframes * WAVES // mk.GRID_WAVES


def test_a_wave_of_every_fold_case_would_wrap_without_its_fold():
    """Per wave and int32 partial, at bytes of -128: squares beyond 2^31, in passes or rows beyond the fold."""
    run, shuffled, per_column = rg.FOLD_CASES
    for fold in rg.FOLD_CASES:
        full = mk.split(*fold.geom, fold.nframes, 0, fold.geom[4], False)
        small = mk.split(*fold.geom, _scaled(fold), 0, fold.geom[4], False, waves=WAVES)
        assert (full.per, full.nseg, full.mode) == (small.per, small.nseg, fold.mode)
        assert full.ranges == mk.GRID_WAVES and small.ranges == WAVES and full.nwork % full.per == 0
    s = mk.split(*run.geom, run.nframes, 0, run.geom[4], False)
    assert (s.nwork, s.per, s.nseg) == (393216, 96, 2)
    skip = mk.skipped_items(s, np.zeros(run.nframes, np.int64), run.geom[4])
    assert skip[1::2].all() and not skip[::2].any()             # the second item of every (aligned) run is empty
    passes = s.per // 2 * (mk.RUN_STEPS // mk.U)
    assert passes == 192 == 3 * mk.RUN_FOLD and passes < 8 * mk.RUN_FOLD
    assert passes * mk.U * mk.STEP // 4 * 128 * 128 == 3 << 30  # one byte phase of the 64 lanes: 1.5 * 2^31
    s = mk.split(*shuffled.geom, shuffled.nframes, 0, shuffled.geom[4], False)
    assert (s.nwork, s.per, s.NV, s.chunk_rows) == (786432, 192, 2, 1024)
    assert s.per * s.chunk_rows == 3 * mk.ROW_FOLD and s.per * s.chunk_rows * 128 * 128 > 1 << 31
    s = mk.split(*per_column.geom, per_column.nframes, 0, per_column.geom[4], False)
    assert (s.per, s.NV, s.rpl, s.chunk_rows, s.units) == (4097, 64, 1, 32, 1)
    assert mk.ROW_FOLD < s.per * s.chunk_rows == 131104 < 8 * mk.ROW_FOLD and 131104 * 128 * 128 > 1 << 31 > 131072 * 127 * 127


def _fold_verdict(fold, value, bin_rows, fault=None):
    layout, npol, nchan, ncomp, ntime = fold.geom
    nframes = _scaled(fold)
    buf = rg.fold_payload(fold, value)
    want = rg.fold_expected(fold, value, nframes, bin_rows or nframes * ntime)
    got = mk.model(buf, np.zeros(nframes, np.int64), *fold.geom, 0, ntime, bin_rows or nframes * ntime, len(want),
                   waves=WAVES, fault=fault, buf_align=fold.buf_align)
    return np.array_equal(got, np.broadcast_to(want[:, None, None, None, :], got.shape))


@pytest.mark.parametrize('fold', rg.FOLD_CASES, ids=lambda f: f.name)
def test_the_fold_cases_catch_a_missing_and_a_late_fold(fold):
    for value in rg.FOLD_VALUES:
        assert _fold_verdict(fold, value, None)
    assert _fold_verdict(fold, -128, rg.FOLD_BIN)
    for fault in ('no_fold', 'fold_x8'):
        assert not _fold_verdict(fold, -128, None, fault), fault
        if fold.name != 'rows-lane-per-column':                 # (there 131104 rows of 127 * 127 stay below 2^31)
            assert not _fold_verdict(fold, 'both', None, fault), fault


def test_the_small_launches_catch_no_late_fold():
    """What the suite had before: sums beyond 32 bits, but four passes a wave -- a fold 8 times too late passes."""
    n = (1 << 17) + 1
    buf = np.full(n * 4, 0x80, np.uint8)
    want = np.zeros((2, 2, 1, 2, 2), np.int64)
    want[0, ..., 0], want[0, ..., 1] = -128 * n, 128 * 128 * n
    for fault in (None, 'fold_x8', 'no_fold'):
        assert np.array_equal(mk.model(buf, [0], CF, 2, 1, 2, n, 0, n, n, 2, fault=fault), want), fault
