"""bb_recode_frames_tables / bb_recode_tables_check without a device: the bound symbols, the
check against bb_recode_check over every width pair and thread shape, and the three refusals
the entry adds -- d_tables NULL, d_tables off a dword, tables too short -- with their order
after everything bb_recode_frames refuses.  The calls carry made-up device addresses, so they
are replayed in a child process that sees no device (tests/abi_replay.py): a check that went
missing shows as BB_EIO, never as a launch."""
import json
import os
import subprocess
import sys

import pytest

import abi_replay
from baseband_amd import _lib, kernels
from conftest import ROOT
from recodekit import WIDTHS, THREAD_SHAPES, fits

OK, E, R, N, IO = _lib.BB_OK, _lib.BB_EINVAL, _lib.BB_ERANGE, _lib.BB_ENOTSUP, _lib.BB_EIO


def test_symbols_are_bound_and_the_version_stays():
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert {'bb_recode_frames_tables', 'bb_recode_tables_check'} <= bound
    assert _lib.lib.bb_abi_version() == 7
    for name in ('bb_recode_frames_tables', 'bb_recode_tables_check'):      # outside the recorded table's patterns
        assert not name.startswith(('bb_decode_', 'bb_encode_'))
        assert not name.endswith(('_scan', '_scan_at', '_locate', '_read_window'))


def payload(bps, chunk):
    return max(4, chunk * bps // 8)


def test_the_check_answers_what_bb_recode_check_answers():
    n = 0
    for bi in WIDTHS:
        for bo in WIDTHS:
            for (si, ci), (so, co) in THREAD_SHAPES:
                for k in (1, 3, 250):
                    args = (bi, bo, ci, si, co, so, k * payload(bi, ci), 5 * k * payload(bo, co))
                    want = _lib.recode_check(*args)
                    assert _lib.recode_tables_check(*args) == want, args
                    assert want == (OK if fits(bi, bo, si * ci) else N)
                assert kernels.recode_tables_supported(bi, bo, ci, si, co, so) == fits(bi, bo, si * ci)
                n += 1
    assert n == 16 * len(THREAD_SHAPES)
    # and on blocks it refuses, the inline map's check among them
    good = dict(bps_in=8, bps_out=2, chunk_in=1, nslot_in=8, chunk_out=4, nslot_out=2, payload_in=1000, payload_out=520)
    for kw in (dict(bps_in=3), dict(reserved=1), dict(chunk_in=3), dict(nslot_out=4), dict(payload_in=1001),
               dict(fill_code=4), dict(row_lo=9, row_hi=8), dict(nslot_in=32, chunk_in=2, nslot_out=2, chunk_out=32)):
        g = dict(good, **kw)
        assert _lib.recode_tables_check(**g) == _lib.recode_check(**g) != OK, kw
    p = _lib.recode_params(table=[4] * 256, **good)
    assert _lib.lib.bb_recode_tables_check(p) == _lib.lib.bb_recode_check(p) == E


# 8 slots of one 8-bit code -> 4 slots of two 2-bit codes; rows: a byte of every input slot, half a byte of every output slot
NFRAMES, PAY_IN, PAY_OUT = 5, 1000, 520
TOTAL = NFRAMES * PAY_IN
BUF, SRC, TAB, OUT = 0x7f0000000000, 0x7f0100000000, 0x7f0200000000, 0x7f0300000000     # made up
BUF_N = NFRAMES * 8 * PAY_IN
TAB_N = 8 << 8
OUT_N = -(-TOTAL // (PAY_OUT * 8 // 2 // 2)) * 4 * PAY_OUT
BLOCK = dict(bps_in=8, bps_out=2, chunk_in=1, nslot_in=8, chunk_out=2, nslot_out=4, fill_code=1, reserved=0,
             payload_in=PAY_IN, payload_out=PAY_OUT, src0=0, src_stride=PAY_IN, row_lo=0, row_hi=TOTAL, first_row=0)


def case(name, buf=BUF, buf_n=BUF_N, src=SRC, nframes=NFRAMES, tab=TAB, tab_n=TAB_N, out=OUT, out_n=OUT_N, block=True, **kw):
    params = {'struct': 'RecodeParams', 'f': dict(BLOCK, **kw)} if block else None
    return {'id': name, 'fn': 'bb_recode_frames_tables',
            'args': [buf, buf_n, src, nframes, params, tab, tab_n, out, out_n, None]}


CASES = [
    # everything in place: the call gets as far as the device, which is not there
    (IO, case('all good')), (IO, case('fixed stride', src=None)), (IO, case('tables longer than needed', tab_n=TAB_N + 5)),
    # the three refusals, each alone
    (E, case('tables NULL', tab=None)), (E, case('tables off a dword', tab=TAB + 2)), (E, case('tables off by one', tab=TAB + 1)),
    (R, case('tables short', tab_n=TAB_N - 1)), (R, case('no tables', tab_n=0)),
    # ... after everything bb_recode_frames refuses: one of its refusals with another code, and a new one
    (N, case('a width | tables NULL', tab=None, bps_out=3)),
    (N, case('whole bytes | tables NULL', tab=None, row_lo=1)),
    (N, case('whole bytes | tables off a dword', tab=TAB + 2, row_lo=1)),
    (R, case('rows beyond the frames | tables NULL', tab=None, row_hi=TOTAL + 4)),
    (R, case('output too small | tables NULL', tab=None, out_n=16)),
    (R, case('output too small | tables off a dword', tab=TAB + 2, out_n=16)),
    (R, case('last fixed-stride payload outside | tables NULL', tab=None, src=None, src_stride=PAY_IN + 4)),
    (E, case('out NULL | tables short', out=None, tab_n=0)),
    (E, case('buf NULL | tables short', buf=None, tab_n=0)),
    (E, case('out off 16 bytes | tables short', out=OUT + 4, tab_n=0)),
    (E, case('reserved | tables short', reserved=1, tab_n=0)),
    (E, case('fixed stride off a dword | tables short', src=None, src0=2, tab_n=0)),
    (N, case('whole bytes | tables short', row_hi=TOTAL - 1, tab_n=0)),
    # ... and among themselves: NULL and alignment before the length
    (E, case('tables NULL | tables short', tab=None, tab_n=0)),
    (E, case('tables off a dword | tables short', tab=TAB + 2, tab_n=TAB_N - 1)),
    # nothing asked for: BB_OK whatever the buffers and tables are, as in bb_recode_frames
    (OK, case('an empty range', tab=None, tab_n=0, row_lo=8, row_hi=8)),
    (OK, case('no frames', tab=None, tab_n=0, nframes=0, row_hi=0)),
    # NULL everything
    (E, case('NULL everything', None, 0, None, 0, None, 0, None, 0, block=False)),
]


@pytest.fixture(scope='module')
def answers(tmp_path_factory):
    table = tmp_path_factory.mktemp('abi') / 'recode_tables_calls.json'
    table.write_text(json.dumps({'cases': [c for _, c in CASES]}))
    env = dict(os.environ, **abi_replay.NO_DEVICE_ENV)
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(ROOT, 'tests', 'abi_replay.py'), str(table)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_ids_are_distinct():
    assert len({c['id'] for _, c in CASES}) == len(CASES)


@pytest.mark.parametrize('code,call', CASES, ids=[c['id'] for _, c in CASES])
def test_refusals_and_their_order(answers, code, call):
    assert answers[call['id']] == code


def test_null_blocks_never_reach_a_device():
    assert _lib.lib.bb_recode_tables_check(None) == E
    assert _lib.lib.bb_recode_frames_tables(None, 0, None, 0, None, None, 0, None, 0, None) == E
