"""What the packed-byte test modules share (statistics, repack, requantize, their readers):
fields of payload bytes to codes and back, buffers with an index over them, the verdict on
a poisoned output.  A plain helper module, imported by name; no test imports another
test module for these."""
import numpy as np

import guardkit


def _torch():
    import torch
    return torch


def unpack_codes(raw, bps):
    """The raw codes of payload bytes, fields LSB first: code e is field e % (8/bps) of
    byte e / (8/bps) (vdif/payload.py:25-103, mark5b/payload.py:27-94)."""
    raw = np.asarray(raw, np.uint8).ravel()
    shifts = np.arange(0, 8, bps, dtype=np.uint8)
    return ((raw[:, None] >> shifts) & ((1 << bps) - 1)).ravel()


def pack_codes(codes, bps):
    """Fields LSB first -> bytes: the inverse of unpack_codes."""
    c = np.asarray(codes, np.uint8).reshape(-1, 8 // bps)
    return (c << np.arange(0, 8, bps, dtype=np.uint8)).sum(1).astype(np.uint8)


def device(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def whole_rows(nbytes, bps, chunk):
    unit = max(4, chunk * bps // 8)
    return -(-nbytes // unit) * unit


def indexed_case(rng, payload, nframes, nslot):
    """A buffer of payloads 20 bytes apart, three of them at odd byte addresses, and an
    index over them: shuffled, with missing entries and entries that leave the buffer."""
    n = nframes * nslot
    step = payload + 20
    buf = rng.integers(0, 256, 16 + n * step, dtype=np.uint8)
    src = 16 + np.arange(n, dtype=np.int64) * step
    src[1 % n] += 1
    src[2 % n] += 2
    src[3 % n] += 3
    rng.shuffle(src)
    bad = [-1, -1, len(buf) - payload + 4, -(1 << 33), len(buf) + (1 << 40)]
    for k, b in zip(rng.choice(n, size=min(n - 1, len(bad)), replace=False), bad):
        src[k] = b
    return buf, src


def judge(whole, view, want, what):
    """Exact bytes; nothing outside the view; words the request does not meet still poison."""
    words = np.ascontiguousarray(want).view(np.uint32)
    v = guardkit.verdict(whole, view, words)
    untouched = int((words == guardkit.POISON).sum())
    assert not v.touched and v.wrong == 0 and v.poison_left == untouched, \
        (what, guardkit.describe(v, words.size), 'words that must stay poison: {}'.format(untouched))
