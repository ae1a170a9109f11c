"""The host arithmetic of the packed-byte path (baseband_amd/base/packed.py) and the
parameter-block builders of its kernels, against brute force.  No device: the validity
marks run on CPU tensors."""
import numpy as np
import pytest
import torch

from baseband_amd import _lib
from baseband_amd.base.packed import _ValidityMarks, piece_rows, samples_per_byte


def _pieces(first, last, per):
    return [(s, min(last, s + per)) for s in range(first, last, per)]


@pytest.mark.parametrize('spf', [1, 5, 8])
def test_request_rows_cover_the_samples_once_and_in_order(spf):
    for start in range(0, 2 * spf + 1):
        for count in range(1, 3 * spf + 1):
            stop = start + count
            first, last = start // spf, (stop - 1) // spf + 1                 # the sets of the first and last sample
            for per in {1, 2, last - first}:
                covered = []
                for s, e in _pieces(first, last, per):
                    row_lo, row_hi, first_row = piece_rows(start, stop, spf, s, e)
                    assert 0 <= row_lo <= row_hi <= (e - s) * spf, (start, count, s, e, row_lo, row_hi)
                    assert first_row == len(covered), (start, count, s, e, first_row)
                    covered += range(s * spf + row_lo, s * spf + row_hi)
                assert covered == list(range(start, stop)), (start, count, per)


def _holes(first, last):
    mid = (first + last) // 2
    return {'first': [first], 'last': [last - 1], 'adjacent': [mid - 1, mid], 'none': []}


@pytest.mark.parametrize('nslot', [1, 3])
@pytest.mark.parametrize('spf,spf_out', [(5, 3), (8, 32), (32, 8), (4, 4)])
def test_validity_marks_against_a_loop(spf, spf_out, nslot):
    for start in (0, spf + spf // 2):
        count = 4 * max(spf, spf_out) + 1
        while count % spf_out == 0:
            count += 1                                                        # (ends inside an output frame)
        stop = start + count
        nout = -(-count // spf_out)
        first, last = start // spf, (stop - 1) // spf + 1
        assert last - first >= 4
        for name, holed in _holes(first, last).items():
            src = np.arange((last - first) * nslot, dtype=np.int64).reshape(last - first, nslot) * 64
            for k in holed:
                src[k - first, k % nslot] = -1
            want = np.array([not any((start + i) // spf in holed
                                     for i in range(k * spf_out, min((k + 1) * spf_out, count))) for k in range(nout)])
            assert want.all() == (not holed)
            for per in (last - first, 1):
                marks = _ValidityMarks(nout, spf_out, start, stop, spf, nslot)
                for s, e in _pieces(first, last, per):
                    marks.add(torch.from_numpy(src[s - first:e - first].reshape(-1).copy()), s, e)
                got = marks.valid()
                assert got.dtype == bool and got.shape == (nout,)
                assert np.array_equal(got, want), (name, start, per, got, want)


def test_samples_per_byte():
    for bps in (1, 2, 4, 8):
        for chunk in (1, 2, 4, 8, 16):
            want = next(n for n in range(1, 9) if n * chunk * bps % 8 == 0)   # the fewest samples that end on a byte
            assert samples_per_byte(chunk, bps) == want, (bps, chunk)


def _fields(p):
    return {name: getattr(p, name) for name, _ in p._fields_}


def test_parameter_block_builders_field_by_field():
    assert _fields(_lib.states_params(2, 4, 8, 8000, 32, 8032, 5, 77, 1)) == dict(
        bps=2, chunk=4, nslot=8, reserved=1, payload_nbytes=8000, src0=32, src_stride=8032, row_lo=5, row_hi=77)
    assert _fields(_lib.states_params(8)) == dict(
        bps=8, chunk=1, nslot=1, reserved=0, payload_nbytes=4, src0=0, src_stride=0, row_lo=0, row_hi=0)
    assert _fields(_lib.states_params(1, row_hi=1 << 63, src0=-4)) == dict(
        bps=1, chunk=1, nslot=1, reserved=0, payload_nbytes=4, src0=-4, src_stride=0, row_lo=0, row_hi=1 << 63)
    assert _fields(_lib.repack_params(2, 0, 1, 4, 8, 32, 1, 8000, 10000, 3, 32, 8032, 8, 800, 16, 1)) == dict(
        bps=2, coder_in=0, coder_out=1, chunk_in=4, nslot_in=8, chunk_out=32, nslot_out=1, fill_code=3,
        payload_in=8000, payload_out=10000, src0=32, src_stride=8032, row_lo=8, row_hi=800, first_row=16, reserved=1)
    assert _fields(_lib.repack_params(1, 1, 0, 1, 2, 2, 1, 64, 128)) == dict(
        bps=1, coder_in=1, coder_out=0, chunk_in=1, nslot_in=2, chunk_out=2, nslot_out=1, fill_code=0,
        payload_in=64, payload_out=128, src0=0, src_stride=0, row_lo=0, row_hi=0, first_row=0, reserved=0)
