"""bb_recode_frames / bb_recode_check without a device: the parameter block's layout, the
bound symbols, every geometry the check takes, every one it refuses, and the order in
which it refuses."""
import ctypes

import pytest

from baseband_amd import _lib, kernels
from recodekit import WIDTHS, THREAD_SHAPES, fits

OK, E, N = _lib.BB_OK, _lib.BB_EINVAL, _lib.BB_ENOTSUP


def test_struct_layout():
    S = _lib.RecodeParams
    assert ctypes.sizeof(S) == 344
    want = dict(bps_in=0, bps_out=4, chunk_in=8, nslot_in=12, chunk_out=16, nslot_out=20, fill_code=24, reserved=28,
                payload_in=32, payload_out=40, src0=48, src_stride=56, row_lo=64, row_hi=72, first_row=80, map=88)
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == want
    assert [n for n, _ in S._fields_] == list(want)
    assert S.map.size == 256


def test_symbols_are_bound():
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {'bb_recode_frames', 'bb_recode_check'} <= bound
    assert _lib.lib.bb_abi_version() == 7


def test_parameter_block_builder_field_by_field():
    p = _lib.recode_params(8, 2, 1, 8, 4, 2, 8000, 2000, range(256), 3, 32, 8032, 8, 800, 16, 1)
    got = {name: getattr(p, name) for name, _ in p._fields_ if name != 'map'}
    assert got == dict(bps_in=8, bps_out=2, chunk_in=1, nslot_in=8, chunk_out=4, nslot_out=2, fill_code=3, reserved=1,
                       payload_in=8000, payload_out=2000, src0=32, src_stride=8032, row_lo=8, row_hi=800, first_row=16)
    assert list(p.map) == list(range(256))
    p = _lib.recode_params(2, 8, 8, 1, 1, 8, 4, 16, [10, 92, 163, 245])
    assert list(p.map) == [10, 92, 163, 245] + [0] * 252 and p.fill_code == 0 and p.row_hi == 0 and p.reserved == 0
    for bad in ([0] * 257, [256], [-1]):
        with pytest.raises(ValueError):
            _lib.recode_params(8, 8, 1, 2, 2, 1, 4, 4, bad)


def payload(bps, chunk):
    return max(4, chunk * bps // 8)


def test_check_takes_every_pair_of_widths_at_every_thread_shape_within_the_limits():
    n = 0
    for bi in WIDTHS:
        for bo in WIDTHS:
            for (si, ci), (so, co) in THREAD_SHAPES:
                if not fits(bi, bo, si * ci):
                    assert not kernels.recode_supported(bi, bo, ci, si, co, so)
                    continue
                for k in (1, 3, 250):
                    rc = _lib.recode_check(bi, bo, ci, si, co, so, k * payload(bi, ci), 5 * k * payload(bo, co),
                                           [(1 << bo) - 1] * (1 << bi), (1 << bo) - 1, 0, 8)
                    assert rc == OK, (bi, bo, si, ci, so, co, k)
                assert kernels.recode_supported(bi, bo, ci, si, co, so)
                n += 1
    assert n == sum(1 for bi in WIDTHS for bo in WIDTHS for (si, ci), _ in THREAD_SHAPES if si * ci * max(bi, bo) <= 256)
    assert n > 100
    assert kernels.RECODE_MAX_ROW_BITS == 256 and kernels.RECODE_MAX_SLOTS == 32


GOOD = dict(bps_in=8, bps_out=2, chunk_in=1, nslot_in=8, chunk_out=4, nslot_out=2, payload_in=1000, payload_out=520,
            table=[3] * 256, fill_code=3, row_lo=0, row_hi=16, first_row=0, reserved=0)


def test_every_refusal():
    assert _lib.recode_check(**GOOD) == OK
    refusals = [
        # 2. a width not in {1, 2, 4, 8}
        (N, dict(bps_in=3)), (N, dict(bps_out=3)), (N, dict(bps_in=0)), (N, dict(bps_out=16)),
        # 3. reserved, a chunk or nslot below 1
        (E, dict(reserved=1)), (E, dict(reserved=-1)), (E, dict(chunk_in=0)), (E, dict(nslot_in=0)),
        (E, dict(chunk_out=0)), (E, dict(nslot_out=-2)),
        # 4. not a power of two
        (N, dict(chunk_in=3, nslot_in=8, chunk_out=3, nslot_out=8)), (N, dict(nslot_in=6, chunk_out=6, nslot_out=1)),
        (N, dict(chunk_out=12, nslot_out=1, chunk_in=12, nslot_in=1)), (N, dict(nslot_out=3, chunk_out=1, nslot_in=3)),
        # 5. the numbers of components differ
        (E, dict(nslot_out=4)), (E, dict(chunk_in=2)),
        # 6. more than 32 slots on a side
        (N, dict(bps_in=2, nslot_in=64, chunk_in=1, nslot_out=1, chunk_out=64, table=[3] * 4, payload_out=512)),
        (N, dict(bps_in=2, nslot_out=64, chunk_out=1, nslot_in=1, chunk_in=64, table=[3] * 4, payload_in=512)),
        # 7. ncomp * max(bps) > 256
        (N, dict(nslot_in=32, chunk_in=2, nslot_out=2, chunk_out=32)),                        # 512 bits of input
        (N, dict(bps_in=1, bps_out=8, nslot_in=1, chunk_in=64, nslot_out=32, chunk_out=2, table=[3, 3],
                 payload_in=64, payload_out=512)),                                             # ... of output
        # 8. payloads
        (E, dict(payload_in=1001)), (E, dict(payload_in=1002)), (E, dict(payload_in=0)),
        (E, dict(payload_out=522)), (E, dict(payload_out=0)),
        (E, dict(chunk_in=8, nslot_in=1, payload_in=1004)),                                   # not whole rows of 8 bytes
        (E, dict(chunk_out=8, nslot_out=1, bps_out=8, payload_out=516)),                      # 64.5 rows of 8 bytes
        # 9. fill_code
        (E, dict(fill_code=4)), (E, dict(fill_code=-1)),
        # 10. a used table entry
        (E, dict(table=[3] * 255 + [4])), (E, dict(table=[255] + [0] * 255)),
        # 11. rows
        (E, dict(row_lo=9, row_hi=8)),
    ]
    for rc, kw in refusals:
        assert _lib.recode_check(**dict(GOOD, **kw)) == rc, kw
        if not set(kw) & {'table', 'fill_code', 'reserved', 'row_lo', 'row_hi'}:
            g = dict(GOOD, **kw)
            assert not kernels.recode_supported(g['bps_in'], g['bps_out'], g['chunk_in'], g['nslot_in'], g['chunk_out'],
                                                g['nslot_out'], g['payload_in'], g['payload_out']), kw
    # entries at index >= 1 << bps_in are ignored
    assert _lib.recode_check(**dict(GOOD, bps_in=2, table=[0, 1, 2, 3] + [255] * 252)) == OK


def test_the_order_of_the_checks():
    """Every adjacent pair of rules that answer different codes, both broken: the earlier
    rule's code.  (Rule 1, the NULL block, has nothing else to break; rules 6 | 7 and 8 .. 11
    answer alike.)"""
    both = [
        (N, dict(bps_in=3, reserved=1)),                                  # 2 before 3
        (N, dict(bps_out=5, chunk_in=0)),
        (E, dict(reserved=1, chunk_in=3)),                                # 3 before 4
        (E, dict(nslot_out=0, nslot_in=6)),
        (N, dict(chunk_in=3)),                                            # 4 before 5: 8 x 3 components against 2 x 4
        (E, dict(bps_in=2, nslot_in=64, chunk_in=1, nslot_out=1, chunk_out=32, table=[3] * 4)),   # 5 before 6: 64 against 32
        (N, dict(nslot_in=32, chunk_in=2, nslot_out=2, chunk_out=32, payload_in=1001)),          # 7 before 8
        (N, dict(nslot_in=32, chunk_in=2, nslot_out=2, chunk_out=32, payload_out=0)),
    ]
    for rc, kw in both:
        assert _lib.recode_check(**dict(GOOD, **kw)) == rc, kw
    # and each of those rules alone, as the later one of its pair
    alone = [(E, dict(reserved=1)), (E, dict(chunk_in=0)), (N, dict(nslot_in=6, chunk_out=6, nslot_out=1)),
             (E, dict(nslot_out=4)), (N, dict(bps_in=2, nslot_in=64, nslot_out=1, chunk_out=64, table=[3] * 4, payload_out=512)),
             (E, dict(payload_in=1001)), (E, dict(payload_out=0))]
    for rc, kw in alone:
        assert _lib.recode_check(**dict(GOOD, **kw)) == rc, kw
    # 6 | 7 and 8 .. 11 answer alike: one call per neighbouring pair still gets that code
    for rc, kw in [(N, dict(bps_in=2, nslot_in=64, chunk_in=8, nslot_out=8, chunk_out=64, table=[3] * 4)),
                   (E, dict(payload_in=1001, fill_code=4)), (E, dict(fill_code=4, table=[4] * 256)),
                   (E, dict(table=[4] * 256, row_lo=9, row_hi=8))]:
        assert _lib.recode_check(**dict(GOOD, **kw)) == rc, kw


def test_null_blocks_never_reach_a_device():
    assert _lib.lib.bb_recode_check(None) == E
    assert _lib.lib.bb_recode_frames(None, 0, None, 0, None, None, 0, None) == E
