"""bb_repack_frames / bb_repack_check (format conversion on the packed bytes): the
parameter block's layout, what the parameters alone decide (no buffers, no device), and
the tie between the code maps the call applies and the pinned oracle's decode-then-encode."""
import ctypes

import numpy as np
import pytest

VDIF, MARK5B, INT = 0, 1, 2
# (coder_in, coder_out) -> the widths the pair has; every one is an exact map from code to code
PAIRS = {(VDIF, VDIF): (1, 2, 4, 8), (MARK5B, MARK5B): (1, 2), (INT, INT): (4, 8),
         (VDIF, MARK5B): (1, 2), (MARK5B, VDIF): (1, 2)}
CODE_MAP = {1: [1, 0], 2: [0, 2, 1, 3]}                     # VDIF <-> Mark 5B, both directions
FILL_CODE = {(VDIF, 1): 1, (VDIF, 2): 2, (MARK5B, 1): 0, (MARK5B, 2): 1}   # the code 0.0 encodes to
POW2 = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def geometries(bps):
    """Every (nslot_in, chunk_in, nslot_out, chunk_out) of powers of two with rows of at most
    256 bits and at most 32 slots on either side."""
    for ncomp in POW2:
        if ncomp * bps > 256:
            continue
        sides = [(ns, ncomp // ns) for ns in POW2 if ns <= 32 and ns <= ncomp]
        for a in sides:
            for b in sides:
                yield a + b


def payload_of(chunk, bps, rows=4):
    unit = max(4, chunk * bps // 8)
    return unit * rows


def test_struct_layout():
    from baseband_amd import _lib
    S = _lib.RepackParams
    assert ctypes.sizeof(S) == 96
    want = dict(bps=0, coder_in=4, coder_out=8, chunk_in=12, nslot_in=16, chunk_out=20, nslot_out=24, fill_code=28,
                payload_in=32, payload_out=40, src0=48, src_stride=56, row_lo=64, row_hi=72, first_row=80,
                reserved=88)
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == want
    assert [n for n, _ in S._fields_] == list(want)


def test_symbols_are_bound():
    from baseband_amd import _lib
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {'bb_repack_frames', 'bb_repack_check'} <= bound
    assert _lib.lib.bb_abi_version() == 7


@pytest.mark.parametrize('bps', (1, 2, 4, 8))
def test_check_takes_every_required_geometry(bps):
    from baseband_amd import _lib
    n = 0
    for ns_in, ch_in, ns_out, ch_out in geometries(bps):
        for (ci, co), widths in PAIRS.items():
            if bps not in widths:
                continue
            rc = _lib.repack_check(bps, ci, co, ch_in, ns_in, ch_out, ns_out, payload_of(ch_in, bps),
                                   payload_of(ch_out, bps, 7), fill_code=(1 << bps) - 1, row_lo=0, row_hi=3)
            assert rc == _lib.BB_OK, (bps, ci, co, ns_in, ch_in, ns_out, ch_out)
            n += 1
    assert n > 100


def test_check_refuses():
    from baseband_amd import _lib
    ok = dict(bps=2, coder_in=VDIF, coder_out=MARK5B, chunk_in=1, nslot_in=8, chunk_out=8, nslot_out=1,
              payload_in=8000, payload_out=5000)

    def ask(**kw):
        return _lib.repack_check(**dict(ok, **kw))

    assert ask() == _lib.BB_OK
    assert ask(bps=3) == _lib.BB_ENOTSUP                                        # no such sample width
    assert ask(bps=4) == _lib.BB_ENOTSUP                                        # Mark 5B has no 4-bit coder
    assert ask(bps=4, coder_out=INT, chunk_out=8) == _lib.BB_ENOTSUP            # VDIF <-> INT needs rescaling
    assert ask(bps=8, coder_in=INT, coder_out=VDIF) == _lib.BB_ENOTSUP
    assert ask(coder_in=INT, coder_out=INT) == _lib.BB_ENOTSUP                  # INT has no 2-bit coder
    assert ask(coder_in=7) == _lib.BB_ENOTSUP
    assert ask(chunk_in=3, nslot_in=8, chunk_out=24) == _lib.BB_ENOTSUP         # not powers of two
    assert ask(nslot_in=3, chunk_in=8, chunk_out=24, payload_out=4992) == _lib.BB_ENOTSUP
    assert ask(nslot_in=64, chunk_out=64) == _lib.BB_ENOTSUP                    # more than 32 slots
    assert ask(nslot_in=1, chunk_in=64, nslot_out=64, chunk_out=1) == _lib.BB_ENOTSUP
    assert ask(chunk_in=32, chunk_out=256, payload_out=4992) == _lib.BB_ENOTSUP  # a row of 512 bits
    for bps in (1, 2):                                                          # rows of 512 bits, every width
        assert ask(bps=bps, nslot_in=1, chunk_in=512 // bps, chunk_out=512 // bps,
                   payload_in=8192, payload_out=8192) == _lib.BB_ENOTSUP
    assert ask(chunk_out=4) == _lib.BB_EINVAL                                   # 8 components in, 4 out
    assert ask(payload_in=8002) == _lib.BB_EINVAL                               # not whole dwords
    assert ask(payload_out=0) == _lib.BB_EINVAL
    assert ask(payload_in=0) == _lib.BB_EINVAL
    assert ask(bps=8, coder_out=VDIF, chunk_in=2, chunk_out=16, payload_out=40) == _lib.BB_EINVAL   # not whole rows
    assert ask(bps=8, coder_out=VDIF, chunk_in=2, chunk_out=16, payload_out=48) == _lib.BB_OK
    assert ask(row_lo=7, row_hi=6) == _lib.BB_EINVAL
    assert ask(row_lo=6, row_hi=6) == _lib.BB_OK
    assert ask(reserved=1) == _lib.BB_EINVAL
    assert ask(fill_code=4) == _lib.BB_EINVAL
    assert ask(fill_code=-1) == _lib.BB_EINVAL
    assert ask(fill_code=3) == _lib.BB_OK
    assert ask(nslot_in=0) == _lib.BB_EINVAL
    assert ask(chunk_out=0) == _lib.BB_EINVAL
    assert _lib.lib.bb_repack_check(None) == _lib.BB_EINVAL


def test_supported_mirrors_the_check():
    from baseband_amd import kernels
    assert kernels.repack_supported(2, VDIF, MARK5B, 1, 8, 8, 1)
    assert kernels.repack_supported(2, MARK5B, VDIF, 8, 1, 1, 8, 10000, 8000)
    assert kernels.repack_supported(8, VDIF, VDIF, 2, 16, 32, 1)
    assert not kernels.repack_supported(8, VDIF, INT, 2, 1, 2, 1)
    assert not kernels.repack_supported(2, VDIF, VDIF, 1, 64, 64, 1)
    assert not kernels.repack_supported(2, VDIF, VDIF, 3, 1, 3, 1)
    assert not kernels.repack_supported(3, VDIF, VDIF, 1, 1, 1, 1)
    assert kernels.REPACK_MAX_ROW_BITS == 256 and kernels.REPACK_MAX_SLOTS == 32


@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_code_maps_are_the_oracle_decode_then_encode(pair):
    """The map the call applies to a code must be what the pinned oracle gives for decode
    in one coder and encode in the other, and the fill codes what it encodes 0.0 to."""
    import bb_oracle_np as orc
    names = {VDIF: 'vdif', MARK5B: 'mark5b', INT: 'int'}
    ci, co = pair
    for bps in PAIRS[pair]:
        codes = np.arange(1 << bps)
        got = orc.encode_codes(orc.code_levels(names[ci], bps), names[co], bps)
        want = codes if ci == co else np.array(CODE_MAP[bps])
        assert np.array_equal(np.asarray(got).astype(np.int64), want), (pair, bps)
    for (coder, bps), code in FILL_CODE.items():
        assert int(np.asarray(orc.encode_codes(np.zeros(1, np.float32), names[coder], bps))[0]) == code
