"""tests/seamkit.py finds the faults it is there to find: driven with seams of 2^15 and 2^16
against NumPy model kernels (no GPU), a correct model passes every helper and each faulty one
-- a source offset truncated to the seam's width, one sign-extended, the last work item above
the seam dropped, a store wrapped to the low addresses -- is caught by every helper it applies
to.  Also the conditions that the inputs of tests/test_seams_gpu.py must meet."""
import numpy as np
import pytest

import bb_oracle_np as orc
import guardkit
import seamkit as sk
from guardkit import GUARD, POISON

LOW, HIGH = 1 << 15, 1 << 16
SIZE = HIGH + (1 << 10)
STRIDE = (1 << 6) + 16                  # the fixed stride, scaled: a multiple of 16, no power of two
UNIT = 24
FILL = np.float32(-2.5)
TABLE = (np.arange(256) - 100.25).astype(np.float32)            # the model's levels: a value per byte
FAULTS = ('truncate', 'sign', 'drop', 'wrap')


def _buffer(seed=1):
    """A buffer whose 'unwritten' bytes differ from anything written later (another generator)."""
    return np.random.default_rng(1000 + seed).integers(0, 256, SIZE, dtype=np.uint8)


def reference(small, index, unit):
    """The plain reference on the compacted units: float32 (unit number, byte)."""
    out = np.empty((len(index), unit), np.float32)
    for k, o in enumerate(index):
        out[k] = TABLE[small[o:o + unit]] if sk.inside(int(o), unit, small.size) else FILL
    return out


def model(buf, src, out, fault=None, item=64, out_seam=HIGH):
    """The model kernel.  Output element e takes TABLE[buf[src[e]]], or FILL where src[e] < 0; work items are
    `item` output elements.  `fault`: what it gets wrong above a seam (LOW / HIGH for source offsets, `out_seam`
    for output elements)."""
    src = np.asarray(src, np.int64).copy()
    e = np.arange(src.size, dtype=np.int64)
    dst = e.copy()
    keep = np.ones(src.size, bool)
    if fault == 'truncate':
        src = np.where(src >= 0, src & (HIGH - 1), src)
    elif fault == 'sign':
        low16 = src & (HIGH - 1)
        src = np.where(src >= 0, np.where(low16 >= LOW, low16 - HIGH, low16), src)
    elif fault == 'drop':
        above = np.flatnonzero((src >= HIGH) | (e >= out_seam))
        if above.size:
            keep[above[-1] // item * item:] = False
    elif fault == 'wrap':
        dst = np.where(e >= out_seam, e - out_seam, e)
    vals = np.where(src >= 0, TABLE[buf[np.clip(src, 0, buf.size - 1)]], FILL).astype(np.float32)
    out[dst[keep]] = vals[keep]


def _unit_sources(index, unit, size):
    """Source offset of every output element of units at `index` (-1: fill)."""
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index <= size - unit)
    return np.where(ok[:, None], index[:, None] + np.arange(unit), -1).reshape(-1)


def _small_output(n):
    whole = sk.allocation(4 * n)
    lo, view = sk.view_of(whole, n, np.float32, 4)
    return whole, lo, view


def test_places():
    p = sk.places(UNIT, SIZE, LOW, HIGH)
    assert len(p) == 11 and p[-1] == -1 and len(set(p)) == 11
    assert p[2] < LOW < p[2] + UNIT and p[3] == LOW                       # straddles the low seam, starts on it
    assert p[4] + UNIT == HIGH and p[5] < HIGH < p[5] + UNIT and p[6] == HIGH
    assert p[7] % 2 == 1 and p[7] >= HIGH + UNIT
    assert p[8] == HIGH + (SIZE - HIGH) // 2
    assert not sk.inside(p[9], UNIT, SIZE) and sk.inside(p[9] - 4, UNIT, SIZE)
    assert all(x % 8 == 0 for x in sk.places(UNIT, SIZE, LOW, HIGH, align=8, odd=False)[:-2])
    full = sk.places(10000)                                               # the defaults: 2^31, 2^32, a tail of 2^26
    assert full[3] == 1 << 31 and full[6] == 1 << 32 and full[8] == (1 << 32) + (1 << 25)
    assert full[9] == sk.SIZE - 10000 + 4 and full[2] == (1 << 31) - 5000
    assert sk.STRIDE % 16 == 0 and sk.STRIDE == (1 << 22) + 64
    n = 1030
    assert 64 + (n - 1) * sk.STRIDE + 16384 <= sk.SIZE and 64 + (n - 2) * sk.STRIDE > sk.HIGH


@pytest.mark.parametrize('fault', (None,) + FAULTS[:3])
def test_sparse_sources(fault):
    buf = _buffer()
    at = sk.places(UNIT, SIZE, LOW, HIGH)
    sp = sk.Sparse(buf, UNIT, at, np.random.default_rng(2))
    small, idx = sp.compact()
    assert small.size < 1024 and len(sp.valid()) == 9
    for k in sp.valid():
        assert idx[k] % 4 == at[k] % 4 and np.array_equal(small[idx[k]:idx[k] + UNIT], buf[at[k]:at[k] + UNIT])
    want = reference(small, idx, UNIT)
    assert (want[9] == FILL).all() and (want[10] == FILL).all() and not (want[:9] == FILL).any()
    whole, lo, view = _small_output(want.size)
    model(buf, _unit_sources(sp.index(), UNIT, SIZE), view, fault, item=UNIT)
    v = guardkit.verdict(whole, view, want)
    assert guardkit.clean(v) == (fault is None), (fault, v)


@pytest.mark.parametrize('fault', (None,) + FAULTS[:3])
def test_fixed_stride(fault):
    buf = _buffer(3)
    n = (SIZE - 16 - UNIT) // STRIDE + 1
    st = sk.Strided(buf, 16, STRIDE, n, UNIT, np.random.default_rng(4))
    assert st.index()[-1] > HIGH and len(st.crossing(LOW)) == 3 and len(st.crossing(HIGH)) == 3
    k = st.crossing(HIGH)[1]
    assert st.index()[k] <= HIGH < st.index()[k] + STRIDE
    small, idx = st.compact()
    assert small.size == n * UNIT and np.array_equal(small[idx[k]:idx[k] + UNIT], buf[st.index()[k]:st.index()[k] + UNIT])
    want = reference(small, idx, UNIT)
    whole, lo, view = _small_output(want.size)
    model(buf, _unit_sources(st.index(), UNIT, SIZE), view, fault, item=UNIT)
    v = guardkit.verdict(whole, view, want)
    assert guardkit.clean(v) == (fault is None), (fault, v)


# a dense output of 2^16 + 2^10 elements; frames of 3 * 24 elements: no seam on a frame boundary
NELEM = HIGH + (1 << 10)
SEAMS = (LOW, HIGH)
NSLOT = 3


def _dense(fault, dtype=np.float32):
    buf = _buffer(5)
    sp = sk.Sparse(buf, UNIT, sk.places(UNIT, SIZE, LOW, HIGH), np.random.default_rng(6))
    small, cidx = sp.compact()
    frame = NSLOT * UNIT
    nframes = NELEM // frame
    live = sk.live_frames(frame, nframes, SEAMS)
    assert len(live) == 6 and any(f * frame < HIGH < (f + 1) * frame for f in live)
    valid = sp.valid()
    idx, used = sk.dense_index(nframes, NSLOT, live, [sp.at[k] for k in valid])
    assert (idx >= 0).sum() == len(live) * NSLOT
    # the model interleaves the slots of a frame set row by row (rows of one byte)
    srcs = _unit_sources(idx, UNIT, SIZE).reshape(nframes, NSLOT, UNIT).transpose(0, 2, 1).reshape(-1)
    ref = reference(small, cidx, UNIT)
    expect = [(f * frame, np.ascontiguousarray(ref[[valid[j] for j in used[f]]].T).astype(dtype)) for f in live]
    n = nframes * frame
    item = np.dtype(dtype).itemsize
    whole = sk.allocation(item * NELEM)
    lo, view = sk.view_of(whole, n, dtype, item)
    if dtype == np.float32:
        model(buf, srcs, view, fault)
    else:
        tmp = np.full(n, np.nan, np.float32)
        model(buf, srcs, tmp, fault)
        done = ~np.isnan(tmp)
        view[done] = tmp[done].astype(dtype)
    return whole, lo, n, item, expect


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
@pytest.mark.parametrize('fault', (None, 'drop', 'wrap'))
def test_dense_output_with_live_frames(fault, dtype):
    whole, lo, n, item, expect = _dense(fault, dtype)
    for _, e in expect:
        assert not guardkit.contains_poison(e)
    fill = np.array([FILL], dtype).view({2: np.uint16, 4: np.uint32}[item])[0]
    v = sk.dense_verdict(whole, lo, n, item, int(fill), expect, chunk=5000)
    assert guardkit.clean(v) == (fault is None), (fault, v)
    if fault == 'drop':
        assert v.poison_left > 0 and v.wrong == 0 and not v.touched
    if fault == 'wrap':
        assert v.poison_left > 0 and v.wrong > 0        # the high frames never stored, and landed on the low ones


def test_dense_verdict_tells_the_faults_apart():
    whole, lo, n, item, expect = _dense(None)
    fill = int(np.array([FILL]).view(np.uint32)[0])
    w = whole.view(np.float32)
    w[lo - 1] = 1.0                                     # a store just before the view
    w[lo + n + 5] = 1.0                                 # ... and behind it
    w[lo + 7] = 3.0                                     # a wrong value where fill belongs
    a, e = expect[-1]
    w[lo + a + 2] += 1                                  # ... and inside a live frame
    whole[lo + 100] = np.array([POISON], np.uint32).view(np.int32)[0]      # an element never stored
    v = sk.dense_verdict(whole, lo, n, item, fill, expect, chunk=4096)
    assert v == ([-1, n + 5], 1, 2)


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
@pytest.mark.parametrize('fault', (None,) + FAULTS)
def test_periodic_data(fault, dtype):
    for P in (7 * 4, 13 * 4):                           # an odd prime number of rows of 4 bytes
        assert all(s % P for s in SEAMS)
        block = np.random.default_rng(P).integers(0, 256, P, dtype=np.uint8)
        buf = np.tile(block, SIZE // P + 1)[:SIZE]
        n = NELEM
        srcs = np.arange(n, dtype=np.int64)
        item = np.dtype(dtype).itemsize
        whole = sk.allocation(item * n)
        lo, view = sk.view_of(whole, n, dtype, item)
        tmp = np.full(n, np.nan, np.float32)
        model(buf, srcs, tmp, fault)
        done = ~np.isnan(tmp)
        view[done] = tmp[done].astype(dtype)
        first = TABLE[block].astype(dtype)
        v = sk.periodic_verdict(whole, lo, n, item, first, chunk=3000)
        if fault == 'sign':
            # offsets in [LOW, HIGH) read as negative: the model then writes FILL, which is no level
            assert v.wrong > 0
        assert guardkit.clean(v) == (fault is None), (fault, P, v)


def test_guards_of_16_bit_views():
    whole = sk.allocation(2 * 1001)
    lo, view = sk.view_of(whole, 1001, np.uint16, 2)    # ends inside a word
    assert sk.guards_touched(whole, lo, 1001, 2) == []
    whole.view(np.uint16)[lo - 3] = 0
    whole.view(np.uint16)[lo + 1001] = 1
    assert sk.guards_touched(whole, lo, 1001, 2) == [1001, -3]
    assert sk._poison_count(whole.view(np.int16)[lo:lo + 1001], lo, 2) == 1001
    view[5] = 0x3C00
    assert sk._poison_count(whole.view(np.int16)[lo:lo + 1001], lo, 2) == 1000


def test_output_seams():
    assert sk.out_seams(4, sk.OUT_ELEMS) == [1 << 29, 1 << 30, 1 << 31, 1 << 32]
    assert sk.out_seams(2, sk.OUT_ELEMS) == [1 << 30, 1 << 31, 1 << 32]
    assert sk.out_seams(1, (1 << 32) + (1 << 20)) == [1 << 31, 1 << 32]
    with pytest.raises(AssertionError):
        sk.live_frames(1 << 12, 1 << 21, [1 << 31])     # a frame boundary on the seam: nothing straddles it


# ---- what the inputs of tests/test_seams_gpu.py must meet ------------------------------------------------

def test_fill_is_no_level_and_not_the_poison():
    import test_seams_gpu as sg
    from test_half_abi import half_bits
    fills = np.array([sg.FILL, sg.M4_FILL], np.float32)
    assert not guardkit.contains_poison(fills)
    for out in (1, 2):
        assert not guardkit.contains_poison(half_bits(fills, out))
    levels = set()
    for coder, bps in sg.CODER_WIDTHS:
        levels |= set(float(x) for x in orc.code_levels(coder, bps))
    levels |= set(float(x) for x in range(-128, 128))                   # int8 casts
    assert not levels & set(float(x) for x in fills)
    # ... nor after rounding to 16 bits
    for out in (1, 2):
        lv = set(int(x) for x in half_bits(np.array(sorted(levels), np.float32), out))
        assert not lv & set(int(x) for x in half_bits(fills, out))
    # A live window of a decode, Mark 4 or int8 case holds levels and the fill and nothing else: none of them is
    # the poison word or one of its halves, so no such window can contain it.  (Windows of copied, encoded and packed
    # bytes are random: test_seams_gpu.py takes the poison word out of its periodic blocks and asserts the rest.)
    everything = np.array(sorted(levels) + [float(x) for x in fills], np.float32)
    assert not guardkit.contains_poison(everything)
    for out in (1, 2):
        assert not guardkit.contains_poison(half_bits(everything, out))


def test_planted_frames_of_the_searches():
    import test_seams_gpu as sg
    for F in (8032, 10016, 40000):
        runs = sg.scan_runs(F)
        assert len(runs) == 8 and sorted(q % 4 for q in runs[:4]) == [0, 1, 2, 3] == sorted(q % 4 for q in runs[4:])
        ends = [(q - sg.SCAN_PAD, q + 3 * F + sg.SCAN_PAD) for q in runs]
        assert all(a[1] <= b[0] + 2 * sg.SCAN_PAD and a[0] + 3 * F < b[0] for a, b in zip(ends, ends[1:]))
        for seam, part in ((sk.LOW, runs[:4]), (sk.HIGH, runs[4:])):
            assert part[0] + 3 * F < seam and part[2] < seam < part[2] + F and part[3] > seam
        assert runs[-1] + 3 * F + sg.SCAN_PAD < sk.SIZE - F


def test_case_lists_are_fixed():
    import test_seams_gpu as sg
    for name, count in sg.CASE_COUNTS.items():
        assert len(getattr(sg, name)) == count, name
    # every frame size of the dense cases lets a frame straddle every seam
    for coder, bps, nslot, chunk, pn in sg.dense_shapes():
        frame = nslot * (pn * 8 // bps)
        for item in (4, 2):
            sk.live_frames(frame, sk.OUT_ELEMS // frame, sk.out_seams(item, sk.OUT_ELEMS))
