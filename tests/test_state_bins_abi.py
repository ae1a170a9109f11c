"""bb_count_states_bins / bb_count_states_bins_check (sampler statistics per time bin):
the symbols, and what the parameters and the bin length alone decide (no buffers, no
device)."""
import ctypes

from test_states_abi import SUPPORTED


def test_symbols_are_bound_and_exported():
    from baseband_amd import _lib
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {'bb_count_states_bins', 'bb_count_states_bins_check'} <= bound
    for name in ('bb_count_states_bins', 'bb_count_states_bins_check'):
        assert getattr(_lib.lib, name) is not None
    assert _lib.lib.bb_abi_version() == 7


def whole_byte_bin(bps, chunk):
    """The shortest legal bin: one row where a row is a byte or more, else one byte."""
    return max(1, 8 // (bps * chunk))


WIDE = [(8, 8), (8, 16)]                                    # more than 1024 counters per bin and slot


def test_check_takes_every_geometry_of_the_unbinned_check_but_the_two_widest():
    from baseband_amd import _lib
    assert set(WIDE) < set(SUPPORTED)
    for bps, chunk in SUPPORTED:
        row_bytes = max(4, chunk * bps // 8)
        assert _lib.count_states_check(bps, chunk, 1, 4 * row_bytes) == _lib.BB_OK
        want = _lib.BB_ENOTSUP if (bps, chunk) in WIDE else _lib.BB_OK
        assert (chunk << bps > 1024) == ((bps, chunk) in WIDE)
        for nslot in (1, 3):
            for bin_rows in (whole_byte_bin(bps, chunk), 1000 * whole_byte_bin(bps, chunk), 2 ** 31 - 8):
                got = _lib.count_states_bins_check(bps, chunk, bin_rows, nslot, 4 * row_bytes, 0, 5)
                assert got == want, (bps, chunk, bin_rows)


def test_check_refuses_what_the_unbinned_check_refuses():
    from baseband_amd import _lib
    ask = _lib.count_states_bins_check
    for bps in (1, 2, 4, 8):                                # chunk * bps = 256
        assert ask(bps, 256 // bps, 8, 1, 64) == _lib.BB_ENOTSUP
    assert ask(2, 24, 8, 1, 48) == _lib.BB_ENOTSUP          # chunk not a power of two
    assert ask(3, 1, 8, 1, 48) == _lib.BB_ENOTSUP           # no such sample width
    assert ask(2, 1, 8, 1, 62) == _lib.BB_EINVAL            # payload not whole dwords
    assert ask(2, 1, 8, 1, 0) == _lib.BB_EINVAL
    assert ask(8, 4, 8, 1, 42) == _lib.BB_EINVAL
    assert ask(2, 1, 8, 1, 8000, 7, 6) == _lib.BB_EINVAL    # row_lo > row_hi
    assert ask(2, 1, 8, 1, 8000, 6, 6) == _lib.BB_OK
    assert ask(2, 1, 8, 1, 8000, reserved=1) == _lib.BB_EINVAL
    assert ask(2, 1, 8, 0, 8000) == _lib.BB_EINVAL
    assert ask(2, 0, 8, 1, 8000) == _lib.BB_EINVAL
    assert _lib.lib.bb_count_states_bins_check(None, 8) == _lib.BB_EINVAL


def test_check_refuses_bin_lengths():
    from baseband_amd import _lib
    ask = _lib.count_states_bins_check
    for bps, chunk in SUPPORTED:
        if (bps, chunk) in WIDE:
            continue
        assert ask(bps, chunk, 0, 1, 128) == _lib.BB_EINVAL
        assert ask(bps, chunk, 2 ** 31, 1, 128) == _lib.BB_EINVAL
        assert ask(bps, chunk, 2 ** 63, 1, 128) == _lib.BB_EINVAL
    assert ask(2, 1, 2 ** 31 - 1, 1, 8000) == _lib.BB_ENOTSUP   # in range, but not whole bytes
    assert ask(2, 1, 2 ** 31 - 4, 1, 8000) == _lib.BB_OK
    assert ask(8, 1, 2 ** 31 - 1, 1, 8000) == _lib.BB_OK
    assert ask(2, 1, 3, 1, 8000) == _lib.BB_ENOTSUP         # bins are whole bytes
    assert ask(2, 1, 4, 1, 8000) == _lib.BB_OK
    assert ask(2, 2, 3, 1, 8000) == _lib.BB_ENOTSUP
    assert ask(2, 2, 2, 1, 8000) == _lib.BB_OK
    assert ask(1, 1, 12, 1, 8000) == _lib.BB_ENOTSUP
    assert ask(1, 4, 3, 1, 8000) == _lib.BB_ENOTSUP
    assert ask(4, 1, 1, 1, 8000) == _lib.BB_ENOTSUP
    assert ask(4, 2, 1, 1, 8000) == _lib.BB_OK
    assert ask(8, 16, 1, 1, 8000) == _lib.BB_ENOTSUP        # 4096 counters per bin
    assert ask(8, 8, 1000, 1, 8000) == _lib.BB_ENOTSUP
    assert ask(8, 4, 1, 1, 8000) == _lib.BB_OK


def test_supported_mirrors_the_check():
    from baseband_amd import _lib, kernels
    for bps, chunk in SUPPORTED:
        for bin_rows in (0, 1, 2, 3, 4, 8, 1000, 2 ** 31 - 1, 2 ** 31):
            row_bytes = max(4, chunk * bps // 8)
            want = _lib.count_states_bins_check(bps, chunk, bin_rows, 1, row_bytes) == _lib.BB_OK
            assert kernels.count_states_bins_supported(bps, chunk, bin_rows) == want, (bps, chunk, bin_rows)
    assert kernels.count_states_bins_supported(2, 16, 1000, 1, 10000)
    assert kernels.count_states_bins_supported(2, 1, 1000, 8, 8000)
    assert not kernels.count_states_bins_supported(2, 1, 1001, 8, 8000)
    assert not kernels.count_states_bins_supported(8, 8, 1000)
    assert not kernels.count_states_bins_supported(2, 12, 1000)
    assert not kernels.count_states_bins_supported(2, 1, -4)
    assert kernels.STATES_BINS_MAX_COUNTERS == 1024


def test_the_struct_is_the_unbinned_call_s():
    from baseband_amd import _lib
    args = dict((n, a) for n, _, a in _lib.SIGNATURES)
    assert args['bb_count_states_bins'][4] is args['bb_count_states'][4]
    assert args['bb_count_states_bins'][5:8] == [ctypes.c_uint64] * 3
    assert args['bb_count_states_bins_check'] == [args['bb_count_states_check'][0], ctypes.c_uint64]
