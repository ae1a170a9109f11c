"""The bytes recorded in tests/golden/launch_notes.json are the oracle's.

Every decode, Mark 4, tiled and copy case of the table is pinned by the SHA-256 of what
the kernels wrote on the GPU the day it was recorded.  Here the same bytes are rebuilt on
the CPU -- tests/launch_expect.py: oracle/bb_oracle_np.decode_flat laid out as
include/bbdecode.h says, the Mark 4 contract, the three transposes -- from the inputs the
replay regenerates, and their digest must equal the recorded one: a wrong answer recorded
that day would otherwise be pinned for good.  No GPU."""
import hashlib
import json

import numpy as np
import pytest

import guardkit
import launch_expect
from conftest import golden_path

with open(golden_path('launch_notes.json')) as _f:
    ALL = json.load(_f)['cases']
CASES = [c for c in ALL if c['op'] in launch_expect.OPS]


def test_the_table_has_202_such_cases():
    # (the 13 encoder cases are pinned to the oracle by tests/test_encode_oracle_gpu.py)
    assert len(CASES) == 202 and len(ALL) - len(CASES) == 13
    assert all(c['op'].startswith('encode') for c in ALL if c not in CASES)


@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_recorded_digest_is_the_oracles(case):
    import launch_replay
    want = launch_expect.expected(case)
    assert want.ndim == 1 and want.size == launch_replay.out_nelem(case)
    assert want.dtype == (np.float32 if case['args'].get('out', 'f32') == 'f32' else np.uint16)
    assert not guardkit.contains_poison(want)
    assert hashlib.sha256(want.tobytes()).hexdigest() == case['sha256']


def test_fill_values_and_levels_are_not_poison():
    import bb_oracle_np as orc
    vals = [launch_expect.DECODE_FILL, launch_expect.TILED_FILL, (launch_expect.MARK4_FILL, 9.0),
            np.arange(-128, 128)]
    vals += [orc.code_levels(c, b) for c, b in (('vdif', 1), ('vdif', 2), ('vdif', 4), ('vdif', 8), ('mark5b', 1),
                                                ('mark5b', 2), ('int', 4), ('int', 8))]
    for v in vals:
        for out in ('f32', 'f16', 'bf16'):
            assert not guardkit.contains_poison(launch_expect.as_out_type(np.asarray(v, np.float32), out))
