"""bb_count_states / bb_count_states_check (sampler statistics): the parameter block's
layout, what the parameters alone decide (no buffers, no device), and the tie between
the raw codes the call counts and the pinned oracle's decoded values."""
import ctypes

import numpy as np
import pytest

from packedkit import unpack_codes


def test_struct_layout():
    from baseband_amd import _lib
    S = _lib.StatesParams
    assert ctypes.sizeof(S) == 56
    want = dict(bps=0, chunk=4, nslot=8, reserved=12, payload_nbytes=16, src0=24, src_stride=32,
                row_lo=40, row_hi=48)
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == want
    assert [n for n, _ in S._fields_] == list(want)


def test_symbols_are_bound():
    from baseband_amd import _lib
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {'bb_count_states', 'bb_count_states_check'} <= bound
    assert _lib.lib.bb_abi_version() == 7


SUPPORTED = [(bps, chunk) for bps in (1, 2, 4, 8) for chunk in (1, 2, 4, 8, 16, 32, 64, 128) if chunk * bps <= 128]


def test_check_takes_every_supported_geometry():
    from baseband_amd import _lib
    assert len(SUPPORTED) == 8 + 7 + 6 + 5
    for bps, chunk in SUPPORTED:
        row_bytes = max(4, chunk * bps // 8)
        for nslot in (1, 3):
            assert _lib.count_states_check(bps, chunk, nslot, 4 * row_bytes, 0, 5) == _lib.BB_OK, (bps, chunk)


def test_check_refuses():
    from baseband_amd import _lib
    ask = _lib.count_states_check
    for bps in (1, 2, 4, 8):                                # chunk * bps = 256
        assert ask(bps, 256 // bps, 1, 64) == _lib.BB_ENOTSUP
    assert ask(2, 24, 1, 48) == _lib.BB_ENOTSUP             # chunk not a power of two
    assert ask(3, 1, 1, 48) == _lib.BB_ENOTSUP              # no such sample width
    assert ask(2, 1, 1, 62) == _lib.BB_EINVAL               # payload not whole dwords
    assert ask(2, 1, 1, 0) == _lib.BB_EINVAL
    assert ask(8, 16, 1, 40) == _lib.BB_EINVAL              # 40 bytes are not whole rows of 16
    assert ask(8, 16, 1, 48) == _lib.BB_OK
    assert ask(2, 1, 1, 8000, 7, 6) == _lib.BB_EINVAL       # row_lo > row_hi
    assert ask(2, 1, 1, 8000, 6, 6) == _lib.BB_OK
    assert ask(2, 1, 1, 8000, reserved=1) == _lib.BB_EINVAL
    assert ask(2, 1, 0, 8000) == _lib.BB_EINVAL
    assert ask(2, 0, 1, 8000) == _lib.BB_EINVAL
    assert _lib.lib.bb_count_states_check(None) == _lib.BB_EINVAL


def test_supported_mirrors_the_check():
    from baseband_amd import kernels
    assert kernels.count_states_supported(2, 16, 1, 10000)
    assert kernels.count_states_supported(8, 16)
    assert not kernels.count_states_supported(8, 32)
    assert not kernels.count_states_supported(2, 12)
    assert kernels.STATES_MAX_ROW_BITS == 128


@pytest.mark.parametrize('coder,name,widths', [(0, 'vdif', (1, 2, 4, 8)), (1, 'mark5b', (1, 2)), (2, 'int', (4, 8))])
def test_codes_and_levels_give_the_oracle_decode(coder, name, widths):
    """Counts are of raw codes: bb_get_levels(coder, bps)[code] must be what the pinned
    oracle decodes the same bytes to, for every coder and width."""
    import bb_oracle_np as orc
    from baseband_amd import _lib
    raw = np.random.default_rng(5).integers(0, 256, 4096, dtype=np.uint8)
    raw[:256] = np.arange(256)
    for bps in widths:
        got = _lib.get_levels(coder, bps)[unpack_codes(raw, bps)]
        want = orc.decode_flat(raw, name, bps)
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, bps)
