"""Pure NumPy helpers of the encoder tests (tests/test_encode_oracle_gpu.py,
tests/test_encode_steps.py): the non-NaN float32 values in ascending order,
the steps of the oracle's encoders found by bisection, inputs that sit on
those steps, and a CPU restatement of the Mark 4 encoder.

Every encoder of `oracle/bb_oracle_np.py` is a step function of its input.
Once that is known to be monotone (`assert_oracle_monotone`), 2^bps - 1
bisections over the ordered floats describe it completely, and a list of the
places where a kernel's code changes can be compared with it exactly."""
import numpy as np

import bb_oracle_np as orc

CODERS = {'vdif': 0, 'mark5b': 1, 'int': 2}
CASES = [('vdif', 1), ('vdif', 2), ('vdif', 4), ('vdif', 8),
         ('mark5b', 1), ('mark5b', 2), ('int', 4), ('int', 8)]

# -inf .. -0.0 and +0.0 .. +inf: 0x7f800001 bit patterns each
HALF = 0x7f800001
NFLOAT = 2 * HALF


def bits_at(pos):
    """Position in ascending float order (0 = -inf, HALF - 1 = -0.0, HALF =
    +0.0, NFLOAT - 1 = +inf) -> float32 bit pattern as uint32."""
    p = np.asarray(pos, dtype=np.int64)
    assert p.size == 0 or (p.min() >= 0 and p.max() < NFLOAT)
    return np.where(p < HALF, 0x80000000 + (HALF - 1 - p), p - HALF).astype(np.uint32)


def floats_at(pos):
    return np.ascontiguousarray(bits_at(pos)).view(np.float32)


def position_of(x):
    """Inverse of `floats_at` (no NaNs)."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    assert b.size == 0 or mag.max() <= 0x7f800000, "NaN has no position"
    return np.where(b >> 31, HALF - 1 - mag, HALF + mag)


def level_order(codes, coder, bps):
    """Code -> rank of the level it stands for (0 = lowest).  The maps are
    involutions, so the same call turns a rank into its code."""
    c = np.asarray(codes).astype(np.int64)
    if coder == 'int':
        return c ^ (1 << (bps - 1))                      # two's complement
    if coder == 'mark5b':
        return np.array([0, 2, 1, 3])[c] if bps == 2 else 1 - c
    return c


def oracle_levels(pos, coder, bps):
    return level_order(orc.encode_codes(floats_at(pos), coder, bps), coder, bps)


_MONOTONE = {}


def assert_oracle_monotone(coder, bps, nsample=1 << 22, seed=0):
    """The oracle's code, in level order, never decreases over a sorted sample
    of `nsample` random float32 values plus the end points and the zeros, and
    runs from level 0 to level 2^bps - 1.  With that, equal codes at the two
    ends of an interval mean one code throughout."""
    key = (coder, bps, nsample, seed)
    if key not in _MONOTONE:
        rng = np.random.default_rng(seed)
        p = rng.integers(0, NFLOAT, nsample, dtype=np.int64)
        # half of the sample where the steps are: |x| < 256
        near = position_of(np.array([-256., 256.], np.float32))
        p[::2] = rng.integers(near[0], near[1], p[::2].size, dtype=np.int64)
        p = np.sort(np.concatenate([p, [0, HALF - 1, HALF, NFLOAT - 1]]))
        lev = oracle_levels(p, coder, bps)
        assert (np.diff(lev) >= 0).all(), (coder, bps)
        assert lev[0] == 0 and lev[-1] == (1 << bps) - 1, (coder, bps, lev[0], lev[-1])
        _MONOTONE[key] = True
    return True


_STEPS = {}


def oracle_steps(coder, bps):
    """(positions, codes) of the oracle's change list: position 0 with the code
    of -inf, then the first position of every later level, by bisection."""
    if (coder, bps) not in _STEPS:
        nlev = 1 << bps
        want = np.arange(1, nlev)
        lo = np.zeros(nlev - 1, np.int64)                # level(lo) < want
        hi = np.full(nlev - 1, NFLOAT - 1, np.int64)     # level(hi) >= want
        assert oracle_levels([0], coder, bps)[0] == 0
        assert oracle_levels([NFLOAT - 1], coder, bps)[0] == nlev - 1
        while (hi - lo > 1).any():
            mid = (lo + hi) // 2
            up = oracle_levels(mid, coder, bps) >= want
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        pos = np.concatenate([[0], hi])
        assert (np.diff(pos) > 0).all(), "a level is skipped"
        codes = level_order(np.arange(nlev), coder, bps).astype(np.uint8)
        assert np.array_equal(orc.encode_codes(floats_at(pos), coder, bps), codes)
        _STEPS[(coder, bps)] = (pos, codes)
    return _STEPS[(coder, bps)]


def codes_from_changes(pos, codes, at):
    """Code a step function given as a change list takes at positions `at`."""
    return np.asarray(codes)[np.searchsorted(np.asarray(pos), at, side='right') - 1]


def neighbours(pos, ulps):
    """All positions within `ulps` of the boundaries `pos` (a boundary is the
    first position of a segment), clipped to the ordered range."""
    p = (np.asarray(pos, np.int64)[:, None] + np.arange(-ulps, ulps, dtype=np.int64)[None, :]).ravel()
    return np.unique(np.clip(p, 0, NFLOAT - 1))


def check_changes(pos, codes, coder, bps, ulps=4096):
    """A kernel's change list (positions, codes) against the oracle: as many
    entries as levels; the oracle agrees at both ends of every segment, one
    position before it, and within `ulps` positions of every boundary."""
    pos = np.asarray(pos, np.int64)
    codes = np.asarray(codes, np.uint8)
    assert_oracle_monotone(coder, bps)
    assert len(pos) == (1 << bps), (coder, bps, len(pos), pos[:20], codes[:20])
    assert pos[0] == 0 and (np.diff(pos) > 0).all()
    last = np.concatenate([pos[1:] - 1, [NFLOAT - 1]])
    for at in (pos, last, np.maximum(pos - 1, 0), neighbours(pos, ulps)):
        want = orc.encode_codes(floats_at(at), coder, bps)
        got = codes_from_changes(pos, codes, at)
        bad = np.nonzero(want != got)[0]
        assert bad.size == 0, (coder, bps, floats_at(at[bad[:8]]), got[bad[:8]], want[bad[:8]])
    opos, ocodes = oracle_steps(coder, bps)
    assert np.array_equal(pos, opos) and np.array_equal(codes, ocodes)


SPECIALS = np.array([np.inf, -np.inf, 0.0, -0.0, 3.4028235e38, -3.4028235e38,
                     1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38], np.float32)
NOISE_SCALE = {1: 1.0, 2: 2.2, 4: 1.4, 8: 1.3}


def noise_scale(coder, bps):
    return NOISE_SCALE[bps] * (30. if coder == 'int' and bps == 8 else 1.)


def step_pool(coder, bps, ulps=16):
    """The floats within `ulps` of every step of a coder, and the specials."""
    pos, _ = oracle_steps(coder, bps)
    return np.concatenate([floats_at(neighbours(pos[1:], ulps)), SPECIALS])


def mixed_input(coder, bps, unit_noise, seed, ulps=16, every=8):
    """`unit_noise` scaled as the encoder tests scale it, with about one sample
    in `every` replaced by a value from `step_pool`."""
    rng = np.random.default_rng(seed)
    x = unit_noise * np.float32(noise_scale(coder, bps))
    pool = step_pool(coder, bps, ulps)
    at = rng.integers(0, x.size, x.size // every)
    x[at] = pool[rng.integers(0, pool.size, at.size)]
    k = min(x.size, pool.size)
    x[:k] = pool[:k]                                     # and every one of them once, up front
    return x


def oracle_packed(x, coder, bps):
    return orc.encode_flat(x, coder, bps) if bps < 8 else orc.encode_codes(x, coder, bps)


def unpack_codes(packed, bps):
    """Packed bytes (first sample in the least significant bits) -> one code per sample."""
    b = np.asarray(packed, np.uint8)
    if bps == 8:
        return b.copy()
    shifts = (np.arange(8 // bps) * bps).astype(np.uint8)
    return ((b[:, None] >> shifts) & ((1 << bps) - 1)).astype(np.uint8).ravel()


M4_WORD = {16: '<u2', 32: '<u4', 64: '<u8'}


def mark4_encode_np(x, ntrack, sign_bit, mag_bit):
    """Mark 4 stream words as bytes for flat float32 `x` (ntrack / 2 values per
    word): the 2-bit VDIF code of value j gives its sign (code >> 1) to track
    bit sign_bit[j] and its magnitude (code & 1) to track bit mag_bit[j]."""
    opw = ntrack // 2
    c = orc.encode_codes(np.asarray(x, np.float32), 'vdif', 2).reshape(-1, opw).astype(np.uint64)
    words = np.zeros(c.shape[0], np.uint64)
    for j in range(opw):
        words |= (c[:, j] >> np.uint64(1)) << np.uint64(sign_bit[j])
        words |= (c[:, j] & np.uint64(1)) << np.uint64(mag_bit[j])
    return words.astype(M4_WORD[ntrack]).view(np.uint8)
