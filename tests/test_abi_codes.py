"""Every argument rule of the C ABI answers the code it answered when
tests/golden/abi_return_codes.json was recorded (oracle/gen_golden_abi_codes.py, at
the commit before the host dispatch was reorganised): one call per rule and entry
point, a single fault each; for the packed-byte entries (bb_count_states,
bb_count_states_bins, bb_repack_frames, bb_requant_frames) also one call per pair of
checks that answer different codes, which holds the order of their checks.

The argument checks run before any HIP call, so no GPU is needed -- and none must be
used: the calls carry made-up device addresses.  They are replayed in a child process
that sees no device and that first makes sure of it (bb_init() answers BB_EIO), so a
check that went missing shows as a wrong code (BB_EIO), never as a launch."""
import json
import os
import subprocess
import sys

import pytest

import abi_replay
from conftest import ROOT, golden_path

TABLE = golden_path('abi_return_codes.json')


@pytest.fixture(scope='module')
def answers():
    env = dict(os.environ, **abi_replay.NO_DEVICE_ENV)
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(ROOT, 'tests', 'abi_replay.py'), TABLE]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def _cases():
    with open(TABLE) as f:
        return json.load(f)['cases']


def test_table_covers_every_checked_entry_point():
    from baseband_amd import _lib
    cases = _cases()
    assert len({c['id'] for c in cases}) == len(cases) >= 300
    assert all(c['code'] != _lib.BB_EIO for c in cases)
    fns = {c['fn'] for c in cases}
    checked = {n for n, _, _ in _lib.SIGNATURES
               if n.startswith(('bb_decode_', 'bb_encode_')) or n.endswith(('_scan', '_scan_at', '_locate', '_read_window'))}
    checked -= {'bb_decode_out_check', 'bb_decode_frames_select_check'}           # (no buffers: tests/test_abi.py, test_half_abi.py)
    checked |= {'bb_copy_frames', 'bb_verify_records', 'bb_build_index', 'bb_mark4_header_crc', 'bb_mark5b_locate_stream',
                'bb_count_states', 'bb_count_states_bins', 'bb_repack_frames', 'bb_requant_frames'}
    assert fns == checked, fns ^ checked
    # an empty request, with a good and with a bad parameter block, for each output type
    for tn in ('f32', 'f16', 'bf16'):
        for what in ('nframes 0', 'nframes 0, payload not whole dwords', 'nframes 0, nslot 0'):
            assert 'bb_decode_frames:{} {}'.format(tn, what) in {c['id'] for c in cases}


def test_every_call_answers_its_recorded_code(answers):
    assert 'error' not in answers, answers
    wrong = {c['id']: (answers.get(c['id']), c['code']) for c in _cases() if answers.get(c['id']) != c['code']}
    assert not wrong, "(got, recorded): {}".format(wrong)
