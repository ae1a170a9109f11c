"""CPU-only checks of tests/encode_steps.py: the float ordering, the oracle's
monotonicity and step counts, and the Mark 4 restatement against the
reference encoders' outputs (tests/golden/encode_cases.npz)."""
import json

import numpy as np
import pytest

import bb_oracle_np as orc
import encode_steps as es
from conftest import golden_path


def test_float_order_is_ascending_and_complete():
    assert es.NFLOAT == 2 * 0x7f800001
    ends = es.floats_at([0, es.HALF - 1, es.HALF, es.NFLOAT - 1])
    assert ends[0] == -np.inf and ends[3] == np.inf
    assert ends.view(np.uint32).tolist() == [0xff800000, 0x80000000, 0x00000000, 0x7f800000]
    rng = np.random.default_rng(1)
    p = np.unique(np.concatenate([rng.integers(0, es.NFLOAT, 1 << 20), np.arange(es.HALF - 3000, es.HALF + 3000),
                                  np.arange(3000), np.arange(es.NFLOAT - 3000, es.NFLOAT)]))
    x = es.floats_at(p)
    assert not np.isnan(x).any()
    assert np.array_equal(es.position_of(x), p)
    # strictly ascending as floats; -0.0 == +0.0 is the one tie
    tie = (p[:-1] == es.HALF - 1) & (p[1:] == es.HALF)
    assert tie.sum() == 1 and ((np.diff(x.astype(np.float64)) > 0) | tie).all()
    # neighbours in position are neighbours in value
    y = np.array([-2.5, -1e-40, 1e-40, 0.75, 3e38], np.float32)
    assert np.array_equal(es.floats_at(es.position_of(y) + 1), np.nextafter(y, np.float32(np.inf)))
    with pytest.raises(AssertionError):
        es.position_of(np.array([np.nan], np.float32))


@pytest.mark.parametrize('coder,bps', es.CASES)
def test_oracle_is_monotone_with_every_level(coder, bps):
    assert es.assert_oracle_monotone(coder, bps)
    pos, codes = es.oracle_steps(coder, bps)
    assert len(pos) == (1 << bps) and len(set(codes.tolist())) == (1 << bps)
    # each boundary is a step of the oracle: the float before it has the previous code
    before = orc.encode_codes(es.floats_at(pos[1:] - 1), coder, bps)
    assert np.array_equal(before, codes[:-1])
    assert np.array_equal(orc.encode_codes(es.floats_at(pos), coder, bps), codes)
    es.check_changes(pos, codes, coder, bps)             # the oracle passes its own comparison


def test_first_steps_are_where_the_arithmetic_puts_them():
    f32 = np.float32
    first = {c: es.floats_at(es.oracle_steps(*c)[0][1:4]) for c in es.CASES}
    assert first[('vdif', 1)].view(np.uint32)[0] == 0x80000000          # -0.0: x >= 0
    assert first[('mark5b', 1)].view(np.uint32)[0] == 0x00000000        # +0.0: signbit
    assert np.array_equal(first[('vdif', 2)], np.array([-2.1745639, -2.3841858e-07, 2.1745639], f32))
    assert np.array_equal(first[('mark5b', 2)], first[('vdif', 2)])
    assert first[('vdif', 4)][0] == f32(-2.5423727)
    # rint is half-to-even: -7.5 -> -8 but -6.5 -> -6
    assert np.array_equal(first[('int', 4)], np.array([-7.4999995, -6.5, -5.4999995], f32))
    assert np.array_equal(first[('int', 8)], np.array([-127.49999, -126.5, -125.49999], f32))


def test_check_changes_rejects_a_moved_or_extra_step():
    pos, codes = es.oracle_steps('int', 4)
    moved = pos.copy()
    moved[2] += 1                                       # -6.5 itself now gets the lower code
    with pytest.raises(AssertionError):
        es.check_changes(moved, codes, 'int', 4)
    extra_p = np.insert(pos, 3, pos[3] - 5)
    extra_c = np.insert(codes, 3, codes[3])
    with pytest.raises(AssertionError):
        es.check_changes(extra_p, extra_c, 'int', 4)
    swapped = codes.copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    with pytest.raises(AssertionError):
        es.check_changes(pos, swapped, 'int', 4)


@pytest.mark.parametrize('coder,bps', es.CASES)
def test_mixed_input_sits_on_the_steps(coder, bps):
    pool = es.step_pool(coder, bps)
    assert pool.size >= 2 * 16 * ((1 << bps) - 1) * 0.9   # neighbourhoods may touch (1-bit: one step)
    noise = np.random.default_rng(3).standard_normal(1 << 16).astype(np.float32)
    x = es.mixed_input(coder, bps, noise.copy(), seed=4)
    assert x.dtype == np.float32 and not np.isnan(x).any()
    assert np.isin(x.view(np.uint32), pool.view(np.uint32)).mean() > 0.1
    assert set(es.unpack_codes(es.oracle_packed(x, coder, bps), bps).tolist()) == set(range(1 << bps))
    c = orc.encode_codes(x, coder, bps)
    assert np.array_equal(es.unpack_codes(es.oracle_packed(x, coder, bps), bps), c)


def test_mark4_restatement_matches_reference_encoders():
    gold = np.load(golden_path('encode_cases.npz'))
    with open(golden_path('mark4_bitmaps.json')) as f:
        maps = json.load(f)
    x = gold['input']
    assert len(maps) == 5
    for name, e in maps.items():
        nchan, fanout, nt = e['nchan'], e['fanout'], e['ntrack']
        n = nchan * fanout * (8192 // (nchan * fanout))
        got = es.mark4_encode_np(x[:n], nt, e['sign_bit'], e['mag_bit'])
        assert np.array_equal(got, gold['mark4_' + name]), name
