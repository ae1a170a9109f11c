"""Replays recorded C-ABI calls (tests/golden/abi_return_codes.json) and reports
the code each one answers.  Used by tests/test_abi_codes.py, in a child process
that sees no device, and by oracle/gen_golden_abi_codes.py, which records the table.

A call is ``{"id", "fn", "args", "code"}``.  An argument is an integer (sizes,
counts and device addresses: the addresses are made up, the argument checks never
follow them), ``null``, ``{"struct": name, "f": {field: value}}`` for a parameter
block passed by reference, or ``{"u8": [...]}`` for a uint8[32] bit map.

    python tests/abi_replay.py TABLE.json      # -> {"id": code, ...} on stdout
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what hides every GPU from the HIP runtime of the child process
NO_DEVICE_ENV = {'HIP_VISIBLE_DEVICES': '-1', 'CUDA_VISIBLE_DEVICES': '-1', 'ROCR_VISIBLE_DEVICES': '-1'}


def _arg(a, keep):
    from baseband_amd import _lib
    if not isinstance(a, dict):
        return a
    if 'u8' in a:
        arr = (C.c_uint8 * 32)(*a['u8'])
        keep.append(arr)
        return arr
    s = getattr(_lib, a['struct'])()
    for name, v in a['f'].items():
        if isinstance(v, list):
            field = getattr(s, name)
            for i, x in enumerate(v):
                field[i] = x
        else:
            setattr(s, name, v)
    keep.append(s)
    return C.byref(s)


def call(case):
    from baseband_amd import _lib
    keep = []
    return getattr(_lib.lib, case['fn'])(*[_arg(a, keep) for a in case['args']])


def device_is_hidden():
    """The replay hands the library made-up addresses: it runs only where a call
    that passes its argument checks stops at the first HIP call."""
    from baseband_amd import _lib
    return _lib.lib.bb_init() == _lib.BB_EIO


def main(path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if not device_is_hidden():
        print(json.dumps({'error': 'bb_init() did not answer BB_EIO: a device is visible, nothing replayed'}))
        return 3
    with open(path) as f:
        cases = json.load(f)['cases']
    print(json.dumps({c['id']: call(c) for c in cases}))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1]))
