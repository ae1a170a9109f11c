"""bb_requant_frames / bb_requant_check without a device: the parameter block's layout, the
bound symbols, every geometry the check takes and every one it refuses."""
import ctypes

import pytest

from baseband_amd import _lib, kernels

OK, E, N = _lib.BB_OK, _lib.BB_EINVAL, _lib.BB_ENOTSUP
WIDTHS = (1, 2, 4, 8)


def test_struct_layout():
    S = _lib.RequantParams
    assert ctypes.sizeof(S) == 336
    want = dict(bps_in=0, bps_out=4, chunk=8, nslot=12, fill_code=16, reserved=20, payload_in=24, payload_out=32,
                src0=40, src_stride=48, row_lo=56, row_hi=64, first_row=72, map=80)
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == want
    assert [n for n, _ in S._fields_] == list(want)
    assert S.map.size == 256


def test_symbols_are_bound():
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {'bb_requant_frames', 'bb_requant_check'} <= bound
    assert _lib.lib.bb_abi_version() == 7


def test_parameter_block_builder_field_by_field():
    p = _lib.requant_params(8, 2, 4, 8, 8000, 2000, range(256), 3, 32, 8032, 8, 800, 16, 1)
    got = {name: getattr(p, name) for name, _ in p._fields_ if name != 'map'}
    assert got == dict(bps_in=8, bps_out=2, chunk=4, nslot=8, fill_code=3, reserved=1, payload_in=8000, payload_out=2000,
                       src0=32, src_stride=8032, row_lo=8, row_hi=800, first_row=16)
    assert list(p.map) == list(range(256))
    p = _lib.requant_params(2, 8, 1, 1, 4, 16, [10, 92, 163, 245])
    assert list(p.map) == [10, 92, 163, 245] + [0] * 252 and p.fill_code == 0 and p.row_hi == 0
    for bad in ([0] * 257, [256], [-1]):
        with pytest.raises(ValueError):
            _lib.requant_params(8, 8, 1, 1, 4, 4, bad)


def payload(bps, chunk):
    return max(4, chunk * bps // 8)


def test_check_takes_every_pair_of_widths_at_every_geometry_within_the_limits():
    n = 0
    for bi in WIDTHS:
        for bo in WIDTHS:
            for nslot in (1, 2, 4, 8, 16, 32):
                for lc in range(9):
                    chunk = 1 << lc
                    if chunk * max(bi, bo) > 256:
                        continue
                    for k in (1, 3, 250):
                        rc = _lib.requant_check(bi, bo, chunk, nslot, k * payload(bi, chunk), 5 * k * payload(bo, chunk),
                                                [(1 << bo) - 1] * (1 << bi), (1 << bo) - 1, 0, 8)
                        assert rc == OK, (bi, bo, nslot, chunk, k)
                    assert kernels.requant_supported(bi, bo, chunk, nslot)
                    n += 1
    assert n == 6 * sum(1 for bi in WIDTHS for bo in WIDTHS for lc in range(9) if (1 << lc) * max(bi, bo) <= 256)
    assert kernels.REQUANT_MAX_ROW_BITS == 256 and kernels.REQUANT_MAX_SLOTS == 32


def test_every_refusal():
    good = dict(bps_in=8, bps_out=2, chunk=2, nslot=8, payload_in=1000, payload_out=520, table=[3] * 256, fill_code=3,
                row_lo=0, row_hi=16, first_row=0, reserved=0)
    assert _lib.requant_check(**good) == OK
    refusals = [
        (N, dict(bps_in=3)), (N, dict(bps_out=3)), (N, dict(bps_in=0)), (N, dict(bps_out=16)),
        (N, dict(chunk=3, payload_in=1002)), (N, dict(chunk=6)), (N, dict(nslot=3)), (N, dict(nslot=12)),
        (N, dict(nslot=64)),
        (N, dict(chunk=64, payload_in=1024)),                       # 512 bits of input
        (N, dict(bps_in=1, bps_out=8, chunk=64, payload_in=64, payload_out=512, table=[3, 3])),   # ... of output
        (E, dict(payload_in=1001)), (E, dict(payload_in=1002)), (E, dict(payload_in=0)),
        (E, dict(payload_out=522)), (E, dict(payload_out=0)),
        (E, dict(chunk=16, payload_in=1000)),                       # 1000 codes are not whole rows of 16
        (E, dict(chunk=128, bps_in=2, table=[3] * 4, payload_in=64, payload_out=48)),   # 192 codes: one and a half rows
        (E, dict(fill_code=4)), (E, dict(fill_code=-1)),
        (E, dict(table=[3] * 255 + [4])), (E, dict(table=[255] + [0] * 255)),
        (E, dict(reserved=1)), (E, dict(reserved=-1)),
        (E, dict(row_lo=9, row_hi=8)),
        (E, dict(chunk=0)), (E, dict(nslot=0)), (E, dict(chunk=-2)),
    ]
    for rc, kw in refusals:
        assert _lib.requant_check(**dict(good, **kw)) == rc, kw
        if not set(kw) & {'table', 'fill_code', 'reserved', 'row_lo', 'row_hi'}:
            g = dict(good, **kw)
            assert not kernels.requant_supported(g['bps_in'], g['bps_out'], g['chunk'], g['nslot'], g['payload_in'],
                                                 g['payload_out']), kw
    # entries at index >= 1 << bps_in are ignored
    assert _lib.requant_check(**dict(good, bps_in=2, payload_in=1000, table=[0, 1, 2, 3] + [255] * 252)) == OK
    assert _lib.lib.bb_requant_check(None) == E
    # nothing with a NULL block reaches the device either
    assert _lib.lib.bb_requant_frames(None, 0, None, 0, None, None, 0, None) == E
