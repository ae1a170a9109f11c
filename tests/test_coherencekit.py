"""tests/coherencekit.py without a device: its oracle against momentkit's and against complex128, the
kernel's dot4 arithmetic against the oracle for every byte value, its constants against the sources, the
split of the small launches, and the sums that the fold cases of tests/test_coherence_kernels_gpu.py rest on."""
import os
import re

import numpy as np
import pytest

import coherencekit as ck
import momentkit as mk
import test_coherence_kernels_gpu as kg
from coherencekit import CF, TF, ROWS

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, 'baseband_amd', 'csrc')


def _defines(name):
    with open(os.path.join(CSRC, name)) as f:
        return dict(re.findall(r'^#define\s+(\w+)\s+(\d+)', f.read(), re.M))


def test_the_constants_are_the_sources():
    d = _defines('k_coherence.h')
    assert (int(d['BB_COH_RUN_FOLD']), int(d['BB_COH_ROW_FOLD'])) == (ck.RUN_FOLD, ck.ROW_FOLD)
    # the shapes in the order of the note's names (bb_packed.inc)
    assert [int(d['BB_COH_' + k]) for k in ('RUN', 'ROW1', 'ROW4', 'SPLIT1', 'SPLIT4')] == [0, 1, 2, 3, 4]
    with open(os.path.join(CSRC, 'bb_packed.inc')) as f:
        text = f.read()
    assert '{"run", "rows4", "rows16", "split4", "split16"}' in text
    m = _defines('k_moments.h')
    assert [int(m[k]) for k in ('BB_MOM_U', 'BB_MOM_STEP', 'BB_MOM_RUN_STEPS', 'BB_MOM_ROW_STEPS')] == [mk.U, mk.STEP, mk.RUN_STEPS, mk.ROW_STEPS]
    assert int(_defines('bb_packed.inc')['BB_MOMENTS_GRID']) * mk.WAVES_PER_BLOCK == mk.GRID_WAVES
    # the lane sum in int32 cannot wrap: a dword adds 2^15 at most, 16 dwords a pass and 64 lanes (run); a row one dword
    assert ck.RUN_FOLD * 16 * 64 << 15 < 1 << 31 <= 2 * ck.RUN_FOLD * 16 * 64 << 15
    assert ck.ROW_FOLD << 15 < 1 << 31 <= 2 * ck.ROW_FOLD << 15


def _payloads(layout, nchan, ntime, nframes, rng):
    pay = ntime * 4 * nchan
    buf = rng.integers(0, 256, 64 + nframes * (pay + 16), dtype=np.uint8)
    buf[64:72] = np.array(ck.EXTREME, np.int8).reshape(-1).view(np.uint8)
    return buf, [64 + k * (pay + 16) for k in range(nframes)]


@pytest.mark.parametrize('layout,nchan', [(CF, 1), (CF, 3), (TF, 1), (TF, 5), (ROWS, 1), (ROWS, 4), (ROWS, 6)])
def test_the_oracle_two_ways(layout, nchan):
    rng = np.random.default_rng([layout, nchan])
    ntime = 50
    buf, offsets = _payloads(layout, nchan, ntime, 3, rng)
    offsets[1] = -1                                            # a missing frame keeps its rows in the series
    for t_lo, t_hi, bin_rows, first_row in ((0, ntime, 7, 0), (3, 45, 1, 5), (1, 2, 100, 0), (0, ntime, 1000, 3)):
        nt = t_hi - t_lo
        nbins = (first_row + 3 * nt - 1) // bin_rows + 1
        got = ck.oracle(buf, offsets, layout, nchan, ntime, t_lo, t_hi, bin_rows, nbins, first_row)
        assert got.shape == (nbins, nchan, 4) and got.dtype == np.int64 and got.any()
        m = mk.oracle(buf, offsets, layout, 2, nchan, 2, ntime, t_lo, t_hi, bin_rows, nbins, first_row)
        assert np.array_equal(got[..., :2], m[..., 1].sum(-1).transpose(0, 2, 1))       # (bin, pol, chan) -> (bin, chan, pol)
        # X * conj(Y) in complex128 from the decoded samples: exact at these sizes
        want = np.zeros((nbins, nchan), np.complex128)
        for f, so in enumerate(offsets):
            if so < 0:
                continue
            s = mk.samples(buf[so:so + ntime * 4 * nchan], layout, 2, nchan, 2, ntime)[t_lo:t_hi].astype(np.float64)
            z = s[..., 0] + 1j * s[..., 1]
            np.add.at(want, (first_row + f * nt + np.arange(nt)) // bin_rows, z[:, 0] * np.conj(z[:, 1]))
        assert np.array_equal(got[..., 2], want.real) and np.array_equal(got[..., 3], want.imag)


def test_the_extreme_quads():
    for quad, sums in zip(ck.EXTREME, ck.EXTREME_SUMS):
        for layout, nchan in ((CF, 2), (TF, 3), (ROWS, 2), (ROWS, 1)):
            buf = ck.constant_payload(layout, nchan, 10, quad)
            got = ck.oracle(buf, [0], layout, nchan, 10, 0, 10, 4, 3)
            assert np.array_equal(got, np.broadcast_to(ck.constant_expected(sums, 10, 4)[:, None, :], got.shape))
    assert ck.EXTREME_SUMS[0][2:] == (128, 32640) and ck.EXTREME_SUMS[1][2:] == (128, -32640)
    assert np.array_equal(ck.constant_expected((1, 2, 3, -4), 10, 4, first_row=3), [[1, 2, 3, -4], [4, 8, 12, -16], [4, 8, 12, -16], [1, 2, 3, -4]])


def test_the_kernels_arithmetic_for_every_byte_value():
    """The five dot products of a quad and the ten of a pair of dwords, as the kernel forms them, against
    plain integer arithmetic: all 65536 (a, b) byte pairs in every position that meets another, -128 included."""
    b = np.arange(256, dtype=np.uint32)
    p, q = (x.reshape(-1) for x in np.meshgrid(b, b, indexing='ij'))
    rng = np.random.default_rng(3)
    r, t = rng.integers(0, 256, (2, p.size), dtype=np.uint32)
    s8 = lambda v: v.astype(np.uint8).view(np.int8).astype(np.int64)      # noqa: E731
    for xr, xi, yr, yi in ((p, r, q, t), (p, r, t, q), (r, p, q, t), (r, p, t, q), (p, q, r, t), (r, t, p, q)):
        a, bb, c, d = s8(xr), s8(xi), s8(yr), s8(yi)
        want = np.stack((a * a + bb * bb, c * c + d * d, a * c + bb * d, bb * c - a * d), -1)
        w = xr | xi << 8 | yr << 16 | yi << 24
        assert np.array_equal(ck.quad_sums(w), want)
        # the same samples as the lower and as the upper channel of a pair of dwords, beside random ones
        x_lo, y_lo = xr | xi << 8 | t << 16 | r << 24, yr | yi << 8 | p << 16 | q << 24
        x_hi, y_hi = t | r << 8 | xr << 16 | xi << 24, p | q << 8 | yr << 16 | yi << 24
        assert np.array_equal(ck.pair_sums(x_lo, y_lo)[:, 0], want) and np.array_equal(ck.pair_sums(x_hi, y_hi)[:, 1], want)
    for quad, sums in zip(ck.EXTREME, ck.EXTREME_SUMS):
        w = np.array(quad, np.int8).view(np.uint32)
        assert ck.quad_sums(w).tolist() == [list(sums)]


def test_split_of_small_launches():
    """What tests/test_coherence_kernels_gpu.py launches."""
    s = ck.split(CF, 65, 1000, 3, 0, 1000, False)
    assert (s.mode, s.nseg, s.units, s.nwork, s.per, s.grid) == ('run', 1, 65, 195, 1, 49)
    s = ck.split(CF, 3, 4200, 3, 0, 4200, True)                   # 16800 bytes a run: two work items
    assert (s.mode, s.nseg, s.nwork) == ('run', 2, 18)
    s = ck.split(TF, 8, 96, 3, 0, 96, True)
    assert (s.mode, s.NV, s.rpl, s.chunk_rows, s.nseg, s.units) == ('rows16', 2, 32, 1024, 1, 1)
    s = ck.split(TF, 4100, 96, 3, 0, 96, False)
    assert (s.mode, s.NV, s.rpl, s.nseg, s.units, s.nwork) == ('rows4', 4100, 1, 3, 65, 585)
    s = ck.split(ROWS, 1, 1001, 3, 0, 1001, True)
    assert s.mode == 'run' and s.units == 1
    for nchan, wide, want in ((2, True, ('split4', 1, 64, 1)), (4, True, ('split4', 2, 32, 1)), (6, True, ('split4', 3, 21, 1)),
                              (8, True, ('split16', 1, 64, 1)), (8, False, ('split4', 4, 16, 1)), (66, True, ('split4', 33, 1, 1)),
                              (72, True, ('split16', 9, 7, 1)), (130, True, ('split4', 65, 1, 2))):
        s = ck.split(ROWS, nchan, 96, 3, 0, 96, wide)
        assert (s.mode, s.NV, s.rpl, s.units) == want, nchan
    assert not ck.supported(ROWS, 3) and ck.supported(ROWS, 1) and ck.supported(TF, 3)


def test_every_range_case_walks_several_items_across_units():
    """The cases of test_ranges_of_many_items, at the stride (an inner row range) and through the index (the
    whole payload): more items than waves, and with several units a range that holds the end of one unit and
    the start of the next; the buffers stay small."""
    for c in kg.RANGE_CASES:
        assert 64 + (c.nframes - 1) * c.stride + c.ntime * 4 * c.nchan < 1 << 20 and ('16' not in c.mode or c.stride % 16 == 0)
        for wide, (t_lo, t_hi) in ((True, (3, c.ntime - 5)), (False, (0, c.ntime))):
            s = ck.split(c.layout, c.nchan, c.ntime, c.nframes, t_lo, t_hi, wide)
            assert s.mode == (c.mode if wide else c.mode.replace('16', '4')), c.name
            assert s.nwork > mk.GRID_WAVES and s.per >= 2, c.name
            assert '16' in c.mode or s.units == c.units
            assert s.units == 1 or (c.nframes * s.nseg) % s.per, c.name
    assert {c.mode for c in kg.RANGE_CASES} == {'run', 'rows4', 'rows16', 'split4', 'split16'}
    assert any(ck.split(c.layout, c.nchan, c.ntime, c.nframes, 0, c.ntime, False).nseg > 1 for c in kg.RANGE_CASES)


def test_a_wave_of_every_fold_case_would_wrap_without_its_fold():
    """Per wave and int32 partial, at the extreme quads: |X|^2 and |Im| beyond 2^31 in passes or rows beyond
    the fold, from buffers of at most 1 MiB."""
    run, rows, split = kg.FOLD_CASES
    per_x, _, _, per_im = ck.EXTREME_SUMS[0]
    for fold in kg.FOLD_CASES:
        s = ck.split(fold.layout, fold.nchan, fold.ntime, fold.nframes, 0, fold.ntime, True)
        assert s.mode == fold.mode and s.ranges == mk.GRID_WAVES and s.nwork % s.per == 0 and s.nwork > 4 * s.grid
        assert fold.ntime * 4 * fold.nchan <= 1 << 20
    s = ck.split(run.layout, run.nchan, run.ntime, run.nframes, 0, run.ntime, True)
    assert (s.nwork, s.per, s.nseg) == (196608, 48, 2)            # the second item of every (aligned) run is empty
    passes = s.per // 2 * (mk.RUN_STEPS // mk.U)
    assert passes == 96 == 3 * ck.RUN_FOLD
    dwords = passes * mk.U * mk.STEP // 4                         # of the wave's 64 lanes
    assert dwords * per_x > 1 << 31 and dwords * per_im > 1 << 31
    for fold, nv in ((rows, 2), (split, 2)):
        s = ck.split(fold.layout, fold.nchan, fold.ntime, fold.nframes, 0, fold.ntime, True)
        assert (s.per, s.NV, s.chunk_rows, s.nseg, s.units) == (96, nv, 1024, 1, 1)
        assert s.per * s.chunk_rows == 3 * ck.ROW_FOLD and s.per * s.chunk_rows * per_x > 1 << 31 < s.per * s.chunk_rows * per_im
