"""Every launch shape of tests/golden/launch_notes.json still leaves the note it left
when the table was recorded (oracle/gen_golden_launch_notes.py, on the GPU, at the
commit before the host dispatch was reorganised) and still writes the same bytes.

The note is the whole bb_last_kernel() string -- kernel, template arguments, grid and
work-item geometry -- compared exactly, where the other tests look for a kernel's name
in it; the output is compared by SHA-256.  The shapes are the smallest at which each
work split, grid cap and dispatch branch can still differ (payloads of 1, 32 and 40
tiles, 64 and 512 frames, BB_TUNE_BLOCKS = 7).  The experiment build words some notes
differently and is not what the table was recorded with."""
import json
import os

import pytest

import launch_replay
from conftest import golden_path

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get('BB_EXPERIMENTS', '') not in ('', '0'),
                                 reason="recorded with the product library (_lib.EXPERIMENTS is set)")]

with open(golden_path('launch_notes.json')) as _f:
    CASES = json.load(_f)['cases']


def test_table_reaches_every_kernel_family():
    notes = ' '.join(c['note'] for c in CASES)
    for kernel in ('k_decode_gather<', 'k_decode_rows_pipe<', 'k_decode_flat_lut<1', 'k_decode_flat_lds<2', 'k_decode_flat_lds<4',
                   'k_decode_flat_lds<8,INT8', 'k_decode_flat_lds<8,LDS', 'k_decode_flat<8,LDS,0', 'k_decode_flat<2,REG,2', 'k_decode_half_flat<1', 'k_decode_half_flat<2', 'k_decode_half_rows<2', 'k_decode_pick<',
                   'k_decode_gather_select<', 'float4', 'scalar', 'k_decode_mark4<16', 'k_decode_mark4<32', 'k_decode_mark4<64',
                   'super-words', 'k_decode_mark4_select<', 'k_decode_i8_xpose<0', 'k_decode_i8_xpose<1', 'k_decode_i8_xpose<2',
                   'k_decode_i8_tf_pick<', 'k_decode_i8_stage<1', 'k_decode_i8_stage<2', 'k_decode_i8_tiled<0', 'k_decode_i8_tiled<1',
                   'k_decode_i8_tiled<2', 'k_copy_frames<nt,16B', 'k_copy_frames<nt,4B', 'k_encode_flat<VDIF,2', 'k_encode_flat<VDIF,4',
                   'k_encode_mark4<'):
        assert kernel in notes, kernel
    # more slots than the gather stages: the rows kernel, or the plain one for rows narrower than a float4
    past = {c['id']: c['note'] for c in CASES if '100 slots' in c['id']}
    assert len(past) == 2 and not any('k_decode_gather' in n for n in past.values())
    assert any(n.startswith('k_decode_flat<2,REG,2') for n in past.values())
    assert any('scalar' in c['note'] and 'k_decode_mark4_select' in c['note'] for c in CASES)


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_launch_leaves_its_recorded_note_and_output(case):
    note, digest = launch_replay.run(case)
    assert note == case['note']
    assert digest == case['sha256']
