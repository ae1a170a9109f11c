"""The encoders (k_encode_flat, k_encode_mark4, kernels.encode_flat /
encode_mark4 and the writers above them) against the NumPy oracle
(oracle/bb_oracle_np.py encode_codes / encode_flat):

A. every non-NaN float32 through every flat coder, reduced on the device to
   the list of places where the code changes, compared on the CPU with the
   oracle at and around every change;
B. every launch shape of k_encode_flat (grid caps, runs per wave, the striped
   work order, tails, the C ABI's answers) byte for byte;
C. k_encode_mark4 against a CPU restatement (tests/encode_steps.py) for
   every mode, word counts around whole waves, grid caps, both 2-bit paths;
D. device views that do not start on a 16-byte boundary, or are not
   contiguous, through the wrappers, the stream writers and the payloads.

Helpers that need no GPU live in tests/encode_steps.py (CPU tests of them:
tests/test_encode_steps.py)."""
import ctypes as C
import io
import json
import time
import warnings

import numpy as np
import pytest

import bb_oracle_np as orc
import encode_steps as es
from conftest import golden_path

pytestmark = pytest.mark.gpu

CASES = es.CASES
CODERS = es.CODERS


def _knobs(**kw):
    """Context manager: set tuning knobs, reset every one of them to 0 on exit."""
    import contextlib
    from baseband_amd import kernels, _lib
    ids = dict(direct=_lib.TUNE_ENCODE_DIRECT, runs=_lib.TUNE_ENCODE_RUNS,
               stripes=_lib.TUNE_ENCODE_STRIPES, blocks=_lib.TUNE_BLOCKS)

    @contextlib.contextmanager
    def cm():
        try:
            for k, v in kw.items():
                kernels.tune(ids[k], v)
            yield
        finally:
            for k in kw:
                kernels.tune(ids[k], 0)
    return cm()


def _both_runs(bps):
    """Is k_encode_flat<.., RUNS = 2> built for this width?  (4-bit codes in the
    product library, every width in the experiment build.)"""
    from baseband_amd import _lib
    return bps == 4 or _lib.EXPERIMENTS


def _name_fields(name):
    """'k_encode_flat<VDIF,2,thresholds,1> grid 64 stripes 0' -> dict."""
    import re
    m = re.match(r'k_encode_flat<(\w+),(\d),(\w+),(\d)> grid (\d+) stripes (\d+)$', name)
    assert m, name
    return dict(coder=m.group(1), bps=int(m.group(2)), path=m.group(3), runs=int(m.group(4)),
                grid=int(m.group(5)), stripes=int(m.group(6)))


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# =============================================================================
# A. every float
# =============================================================================
A_CHUNK = 1 << 28
# the ordered range padded with repeats of +inf to whole 8-byte words of 1-bit codes
A_TOTAL = -(-es.NFLOAT // 64) * 64
A_VARIANTS = ([('%s%d' % c, c[0], c[1], {}) for c in CASES]
              + [('%s2-direct' % c, c, 2, dict(direct=1)) for c in ('vdif', 'mark5b')]
              + [('%s4-runs%d' % (c, r), c, 4, dict(runs=r)) for c in ('vdif', 'int') for r in (1, 2)])
A_MAX_CANDIDATES = 1 << 14         # words per chunk that may hold a change: 256 are expected at most


def _ordered_floats(start, n):
    """float32 device tensor of positions [start, start + n) of the ascending
    order of tests/encode_steps.py (past the end: +inf again)."""
    import torch
    p = torch.arange(start, start + n, dtype=torch.int64, device='cuda').clamp_(max=es.NFLOAT - 1)
    bits = torch.where(p < es.HALF, (0x80000000 + es.HALF - 1) - p, p - es.HALF)
    del p
    return (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)


def _candidate_words(out, bps):
    """The packed output as 8-byte words, and the mask of the words that can
    hold a change of code: word 0, every word that differs from the one before
    it, and every word whose codes are not all the same.  (Every other word
    repeats the last code of its predecessor.)  No synchronisation."""
    import torch
    w = out.view(torch.int64)
    cand = torch.ones(w.numel(), dtype=torch.bool, device=out.device)
    cand[1:] = w[1:] != w[:-1]
    mask = (1 << bps) - 1
    rep = ((1 << 64) - 1) // mask                       # the lowest code, repeated over the word
    cand |= w != (w & mask) * (rep - (1 << 64) if rep >> 63 else rep)
    return w, cand


def _gather_candidates(words, cands):
    """[(word index, word value) as NumPy arrays] for several outputs of one
    chunk, with two synchronisations for all of them."""
    import torch
    sizes = np.cumsum([0] + [c.numel() for c in cands])
    idx = torch.nonzero(torch.cat(cands)).reshape(-1)
    host = idx.cpu().numpy()
    cuts = np.searchsorted(host, sizes)
    vals = torch.cat([w[idx[a:b] - int(lo)] for w, a, b, lo in zip(words, cuts[:-1], cuts[1:], sizes[:-1])])
    vals = vals.cpu().numpy()
    return [(host[a:b] - lo, vals[a:b]) for a, b, lo in zip(cuts[:-1], cuts[1:], sizes[:-1])]


def _bytes_of_words(idx, vals):
    """Word indices and little-endian int64 values -> byte indices and values."""
    by = np.ascontiguousarray(vals.astype('<i8')).view(np.uint8).reshape(-1, 8)
    return (idx[:, None] * 8 + np.arange(8)).ravel(), by.ravel()


class _ChangeList:
    def __init__(self, bps):
        self.bps, self.pos, self.codes, self.prev = bps, [], [], -1

    def add(self, start, idx, vals):
        per, mask = 8 // self.bps, (1 << self.bps) - 1
        for i, b in zip(idx.tolist(), vals.tolist()):
            for k in range(per):
                c = (b >> (k * self.bps)) & mask
                if c != self.prev:
                    p = start + i * per + k
                    assert p < es.NFLOAT, "the code changes inside the +inf padding"
                    self.pos.append(p)
                    self.codes.append(c)
                    self.prev = c
        assert len(self.pos) <= 4 << self.bps, ("far more changes than levels", self.pos[:32], self.codes[:32])


@pytest.fixture(scope='module')
def change_lists():
    """One pass over all ordered floats: each chunk is generated once and goes
    through every variant's launch.  -> {label: (positions, codes)}, and the
    wall time of the pass."""
    import torch
    from baseband_amd import kernels, _lib
    lists = {v[0]: _ChangeList(v[2]) for v in A_VARIANTS}
    errors = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for start in range(0, A_TOTAL, A_CHUNK):
        n = min(A_CHUNK, A_TOTAL - start)
        x = _ordered_floats(start, n)
        if start == 0 or start + n >= A_TOTAL or start <= es.HALF < start + n:
            # the device's enumeration is the CPU helper's
            at = np.unique(np.clip(np.concatenate([np.arange(start, start + 4096), np.arange(start + n - 4096, start + n),
                                                   np.arange(es.HALF - 4096, es.HALF + 4096)]), start, start + n - 1))
            got = x[torch.from_numpy(at - start).cuda()].cpu().numpy()
            want = es.floats_at(np.minimum(at, es.NFLOAT - 1))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        live = [v for v in A_VARIANTS if v[0] not in errors]
        words, cands = [], []
        for label, coder, bps, knobs in live:
            with _knobs(**knobs):
                w, c = _candidate_words(kernels.encode_flat(x, CODERS[coder], bps), bps)
                if start == 0:                            # the variant asked for is the one launched
                    f = _name_fields(_lib.last_kernel())
                    want_runs = 1 if knobs.get('direct') else knobs.get('runs', 2 if bps == 4 else 1)
                    assert (f['bps'], f['path'], f['runs']) == \
                        (bps, 'direct' if knobs.get('direct') else 'thresholds', want_runs), (label, f)
                    assert f['coder'] == coder.upper() and f['stripes'] == 0, (label, f)
            words.append(w)
            cands.append(c)
        del x
        for (label, coder, bps, knobs), (idx, vals) in zip(live, _gather_candidates(words, cands)):
            try:
                assert idx.size <= A_MAX_CANDIDATES, \
                    "%d words of a chunk hold a change of code: the output is no step function" % idx.size
                lists[label].add(start, *_bytes_of_words(idx, vals))
            except AssertionError as exc:                 # that variant's test reports it
                errors[label] = exc
        del words, cands
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    print("\nencode, every float: %d variants x %d values in %.2f s" % (len(A_VARIANTS), es.NFLOAT, elapsed))
    return lists, errors, elapsed


@pytest.mark.parametrize('label,coder,bps,knobs', A_VARIANTS, ids=[v[0] for v in A_VARIANTS])
def test_every_float_encodes_as_the_oracle_says(change_lists, label, coder, bps, knobs):
    """All 2 x 0x7f800001 non-NaN float32 values in ascending order through the
    kernel; the places where its code changes must be the 2^bps the oracle has,
    and the oracle must agree at both ends of every segment, one float before
    it, and at 4096 floats either side of every boundary.  The oracle is
    monotone in level order (checked on 2^22 random floats), so equal end
    points mean a constant segment: together that is every float."""
    lists, errors, _ = change_lists
    if label in errors:
        raise errors[label]
    got = lists[label]
    es.check_changes(got.pos, got.codes, coder, bps, ulps=4096)


def test_two_bit_thresholds_are_the_oracles_boundaries():
    from baseband_amd import _lib
    thr = _lib.encode_thresholds()
    for coder in ('vdif', 'mark5b'):
        pos, _ = es.oracle_steps(coder, 2)
        assert np.array_equal(thr.view(np.uint32), es.floats_at(pos[1:]).view(np.uint32)), (thr, es.floats_at(pos[1:]))


@pytest.mark.parametrize('coder,bps', CASES)
def test_nans_leave_their_neighbours_alone(coder, bps):
    """The reference's integer cast of NaN is undefined, so NaN codes are not
    compared; every other sample of the packed output must be the oracle's."""
    import torch
    from baseband_amd import kernels
    rng = np.random.default_rng(100 + bps)
    n = (1 << 18) + 4 * 9 + (4 if bps == 1 else 0)
    x = es.mixed_input(coder, bps, rng.standard_normal(n).astype(np.float32), seed=bps)
    nan_at = np.unique(np.concatenate([rng.integers(0, n, 3000), [0, 1, 5, 255, 256, 1023, 1024, n - 2, n - 1]]))
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], np.uint32).view(np.float32)
    xn = x.copy()
    xn[nan_at] = nans[rng.integers(0, 4, nan_at.size)]
    assert np.isnan(xn).sum() == nan_at.size
    got = es.unpack_codes(kernels.encode_flat(torch.from_numpy(xn).cuda(), CODERS[coder], bps).cpu().numpy(), bps)
    want = orc.encode_codes(x, coder, bps)                # (x without the NaNs: their codes are masked)
    keep = np.ones(n, bool)
    keep[nan_at] = False
    assert got.shape == want.shape and np.array_equal(got[keep], want[keep])


# =============================================================================
# B. every launch shape of k_encode_flat
# =============================================================================
LWS = (1, 3, 6, 10)
B_RUNS = (64 << 10) + (1 << 10)                    # the largest run count below, rounded up
B_NQUAD = B_RUNS * 256
_noise = {}


def _unit_noise(n):
    if n not in _noise:
        _noise.clear()
        _noise[n] = np.random.default_rng(2024).standard_normal(n, dtype=np.float32)
    return _noise[n]


@pytest.fixture(scope='module')
def big():
    """(coder, bps) -> (input, oracle's packed bytes), both on the device.  The
    encoders work sample by sample, so the expected output of any prefix of
    the input (from a byte boundary on) is that prefix of the bytes."""
    import torch
    cache = {}

    def get(coder, bps):
        if (coder, bps) not in cache:
            x = es.mixed_input(coder, bps, _unit_noise(4 * B_NQUAD), seed=17 * bps + len(coder))
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)      # FLT_MAX * 35.5 overflows, as in the reference
                want = es.oracle_packed(x, coder, bps)
            cache[(coder, bps)] = (torch.from_numpy(x).cuda(), torch.from_numpy(want).cuda())
        return cache[(coder, bps)]
    yield get
    cache.clear()
    _noise.clear()


def _prefix(big, coder, bps, nquad):
    x, want = big(coder, bps)
    return x[:4 * nquad], want[:4 * nquad * bps // 8]


GUARD = 64


def _encode_poisoned(x, coder, bps):
    """bb_encode_flat straight into a fresh buffer prefilled with 0xA5, with a
    guard band either side: bytes a launch leaves unwritten cannot pass as an
    earlier launch's correct output, as they could in a recycled torch.empty."""
    import torch
    from baseband_amd import _lib
    nb = x.numel() * bps // 8
    buf = torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    rc = _lib.lib.bb_encode_flat(C.c_void_p(x.data_ptr()), x.numel(), CODERS[coder], bps,
                                 C.c_void_p(buf.data_ptr() + GUARD), nb, _stream())
    assert rc == _lib.BB_OK, rc
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nb:] == 0xA5).all()), "guard band touched"
    return buf[GUARD:GUARD + nb]


def _even(q, bps):
    """Quad counts of 1-bit data are even (whole bytes)."""
    return q if bps != 1 or q % 2 == 0 else (q + 1 if q == 1 else q - 1)


@pytest.mark.parametrize('coder,bps', CASES)
def test_grid_caps_and_runs_per_wave(big, coder, bps):
    """BB_TUNE_BLOCKS 1, 3, 64 on 2^20 quads and a ragged tail: every wave takes
    16 to 1024 steps of the grid-stride loop, with one and with two runs a step."""
    import torch
    from baseband_amd import kernels, _lib
    nquad = (1 << 20) + _even(37, bps)
    x, want = _prefix(big, coder, bps, nquad)
    with _knobs(runs=1):
        assert torch.equal(_encode_poisoned(x, coder, bps), want)
        plain = _lib.last_kernel()
    assert _name_fields(plain)['runs'] == 1 and _name_fields(plain)['bps'] == bps
    for cap in (1, 3, 64):
        for runs in (1, 2):
            with _knobs(blocks=cap, runs=runs):
                got = _encode_poisoned(x, coder, bps)
                name = _lib.last_kernel()
            assert torch.equal(got, want), (cap, runs, name)
            f = _name_fields(name)
            assert f['grid'] == cap and f['stripes'] == 0
            assert f['runs'] == (runs if _both_runs(bps) else 1), name
    # where RUNS = 2 is not built the knob changes nothing: same kernel, same grid
    with _knobs(runs=2):
        assert torch.equal(_encode_poisoned(x, coder, bps), want)
        two = _lib.last_kernel()
    if _both_runs(bps):
        assert _name_fields(two)['runs'] == 2 and _name_fields(two)['grid'] < _name_fields(plain)['grid']
    else:
        assert two == plain
    with _knobs():
        assert torch.equal(_encode_poisoned(x, coder, bps), want)
        assert _name_fields(_lib.last_kernel())['runs'] == (2 if bps == 4 else 1)


@pytest.mark.parametrize('coder,bps', CASES)
def test_striped_work_order(big, coder, bps):
    """BB_TUNE_ENCODE_STRIPES: one run fewer than the rule needs (input order),
    exactly enough, and enough plus left-over runs past perm.n, each with four
    tails; for 4-bit codes also under a grid cap with two runs a step."""
    import torch
    from baseband_amd import kernels, _lib
    for lw in LWS:
        for nrun in ((64 << lw) - 1, 64 << lw, (64 << lw) + (1 << lw) - 1):
            active = (nrun >> lw) >= 64
            for tail in (1, 2, 63, 255):
                x, want = _prefix(big, coder, bps, nrun * 256 + _even(tail, bps))
                with _knobs(stripes=lw):
                    got = _encode_poisoned(x, coder, bps)
                    name = _lib.last_kernel()
                assert torch.equal(got, want), (lw, nrun, tail, name)
                assert _name_fields(name)['stripes'] == ((1 << lw) if active else 0), name
            if bps == 4:
                x, want = _prefix(big, coder, bps, nrun * 256 + 63)
                with _knobs(stripes=lw, blocks=3, runs=2):
                    got = _encode_poisoned(x, coder, bps)
                    name = _lib.last_kernel()
                assert torch.equal(got, want), (lw, nrun, name)
                f = _name_fields(name)
                assert (f['grid'], f['runs'], f['stripes']) == (3, 2, (1 << lw) if active else 0)


def test_stripes_knob_out_of_range_is_off(big):
    """11 and -1 behave as 0, at a run count where 11 stripes would be dealt."""
    import torch
    from baseband_amd import kernels, _lib
    x, want = big('vdif', 2)
    x, want = torch.cat([x, x]), torch.cat([want, want])
    assert (x.numel() // 1024) >> 11 >= 64
    for value, stripes in ((10, 1024), (11, 0), (-1, 0), (0, 0)):
        try:
            kernels.tune(_lib.TUNE_ENCODE_STRIPES, value)
            got = _encode_poisoned(x, 'vdif', 2)
            name = _lib.last_kernel()
        finally:
            kernels.tune(_lib.TUNE_ENCODE_STRIPES, 0)
        assert torch.equal(got, want), value
        assert _name_fields(name)['stripes'] == stripes, (value, name)



@pytest.mark.parametrize('coder,bps', CASES)
def test_every_tail_length_inside_guard_bands(big, coder, bps):
    """1 to 300 quads (even counts for 1-bit): no whole run up to 255, one run
    and a tail above; the cross-lane pairing of the 1-bit tail and the shuffle
    transpose of the 2-bit run.  Nothing is written outside the output."""
    import torch
    from baseband_amd import _lib
    x, want = big(coder, bps)
    slot = -(-(GUARD + 300 * 4 * bps // 8 + GUARD) // 16) * 16      # (every row's output is aligned)
    counts = [q for q in range(1, 301) if bps != 1 or q % 2 == 0]
    buf = torch.full((len(counts), slot), 0xA5, dtype=torch.uint8, device='cuda')
    exp = buf.clone()
    for row, q in enumerate(counts):
        off = 1024 * q                                   # another stretch of the input each time
        nb = 4 * q * bps // 8
        src = x[off:off + 4 * q]
        rc = _lib.lib.bb_encode_flat(C.c_void_p(src.data_ptr()), 4 * q, CODERS[coder], bps,
                                     C.c_void_p(buf[row].data_ptr() + GUARD), nb, _stream())
        assert rc == _lib.BB_OK, (q, rc)
        exp[row, GUARD:GUARD + nb] = want[off * bps // 8:off * bps // 8 + nb]
    if not torch.equal(buf, exp):
        bad = torch.nonzero((buf != exp).any(dim=1)).reshape(-1).cpu().tolist()
        raise AssertionError("quad counts with wrong bytes or a touched guard band: %r"
                             % [counts[r] for r in bad[:20]])


def test_encode_abi_answers():
    import torch
    from baseband_amd import _lib
    lib = _lib.lib
    x = torch.zeros(1024 + 8, dtype=torch.float32, device='cuda')
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device='cuda')
    xp, op, st = x.data_ptr(), out.data_ptr(), _stream()
    vp = C.c_void_p
    assert xp % 16 == 0 and op % 16 == 0

    def flat(ptr_in, n, coder, bps, ptr_out, nout):
        return lib.bb_encode_flat(vp(ptr_in), n, coder, bps, vp(ptr_out), nout, st)
    for coder, bps in [(c, b) for c in (0, 1, 2) for b in (1, 2, 3, 4, 8, 16)]:
        ok = (('vdif', 'mark5b', 'int')[coder], bps) in CASES
        assert flat(xp, 1024, coder, bps, op, 4096) == (_lib.BB_OK if ok else _lib.BB_ENOTSUP), (coder, bps)
        # zero elements: nothing to do, null pointers are fine -- for a pair the library knows
        assert lib.bb_encode_flat(None, 0, coder, bps, None, 0, None) == (_lib.BB_OK if ok else _lib.BB_ENOTSUP)
    assert flat(xp, 1024, 7, 2, op, 4096) == _lib.BB_ENOTSUP
    assert flat(xp, 1024, -1, 2, op, 4096) == _lib.BB_ENOTSUP
    for coder, bps in CASES:
        c = CODERS[coder]
        nb = 1024 * bps // 8
        assert flat(xp, 1024, c, bps, op, nb) == _lib.BB_OK
        assert flat(xp, 1024, c, bps, op, nb - 1) == _lib.BB_ERANGE
        assert flat(xp, 1024, c, bps, op, 0) == _lib.BB_ERANGE
        for n in (1, 2, 3, 5, 6, 1022, 1023):              # not whole quads
            assert flat(xp, n, c, bps, op, 4096) == _lib.BB_EINVAL, (coder, bps, n)
        if bps == 1:
            assert flat(xp, 4, c, bps, op, 4096) == _lib.BB_EINVAL       # a quad of 1-bit codes is half a byte
            assert flat(xp, 1020, c, bps, op, 4096) == _lib.BB_EINVAL
        for shift in (4, 8, 12):
            assert flat(xp + shift, 1024, c, bps, op, 4096) == _lib.BB_EINVAL, (coder, bps, shift)
        for shift in (1, 2, 3):
            assert flat(xp, 1024, c, bps, op + shift, 4096 - shift) == _lib.BB_EINVAL, (coder, bps, shift)
        assert flat(xp, 1024, c, bps, op + 4, nb) == _lib.BB_OK             # 4-byte aligned output is enough
        assert flat(0, 1024, c, bps, op, 4096) == _lib.BB_EINVAL
        assert flat(xp, 1024, c, bps, 0, 4096) == _lib.BB_EINVAL
    # Mark 4
    with open(golden_path('mark4_bitmaps.json')) as f:
        maps = json.load(f)
    u8 = C.c_uint8 * 32

    def m4(ptr_in, nwords, nt, sb, mb, ptr_out, nout):
        return lib.bb_encode_mark4(vp(ptr_in), nwords, nt, sb, mb, vp(ptr_out), nout, st)
    for e in maps.values():
        nt = e['ntrack']
        sb, mb = u8(*e['sign_bit']), u8(*e['mag_bit'])
        nw = 1024 // (nt // 2)
        nb = nw * nt // 8
        assert m4(xp, nw, nt, sb, mb, op, nb) == _lib.BB_OK
        assert m4(xp, nw, nt, sb, mb, op, nb - 1) == _lib.BB_ERANGE
        assert m4(xp + 4, nw, nt, sb, mb, op, nb) == _lib.BB_EINVAL
        assert m4(xp + 8, nw, nt, sb, mb, op, nb) == _lib.BB_EINVAL
        assert m4(xp, nw, nt, sb, mb, op + 4, nb) == _lib.BB_EINVAL
        assert m4(xp, nw, nt, sb, mb, op + 8, nb) == _lib.BB_OK
        assert m4(0, nw, nt, sb, mb, op, nb) == _lib.BB_EINVAL
        assert m4(xp, nw, nt, None, mb, op, nb) == _lib.BB_EINVAL
        assert lib.bb_encode_mark4(None, 0, nt, None, None, None, 0, None) == _lib.BB_OK
        for which in (0, nt // 2 - 1):
            for bad in (nt, 255):
                s2 = list(e['sign_bit'])
                s2[which] = bad
                assert m4(xp, nw, nt, u8(*s2), mb, op, nb) == _lib.BB_EINVAL, (nt, which, bad)
                m2 = list(e['mag_bit'])
                m2[which] = bad
                assert m4(xp, nw, nt, sb, u8(*m2), op, nb) == _lib.BB_EINVAL, (nt, which, bad)
    e = maps['2_2_4']
    for nt in (0, 8, 24, 48, 128, -16):
        assert m4(xp, 4, nt, u8(*e['sign_bit']), u8(*e['mag_bit']), op, 4096) == _lib.BB_ENOTSUP, nt
        assert lib.bb_encode_mark4(None, 0, nt, None, None, None, 0, None) == _lib.BB_ENOTSUP
    torch.cuda.synchronize()
    # the refused calls wrote nothing past what the accepted ones cover
    assert bool((out[1024 + 8:] == 0xA5).all())


# =============================================================================
# C. k_encode_mark4
# =============================================================================
M4_LARGE = (1 << 20) + 37                          # words


def _m4_word_counts(ntrack):
    """Word counts whose quad count (words x ntrack / 8) is 1, 63, 64, 65,
    4 x 256 x 4 - 1 and + 1 -- or, where that is no whole number of words, the
    whole numbers either side of it: below, at and above one wave, and either
    side of the grid that gives every lane exactly four quads."""
    lpw = ntrack // 8
    counts = set()
    for quads in (1, 63, 64, 65, 4 * 256 * 4 - 1, 4 * 256 * 4 + 1):
        counts.update({max(1, quads // lpw), -(-quads // lpw)})
    return sorted(counts)


def _m4_input(name, e):
    """Noise with one sample in four from the +-4096-ulp neighbourhoods of the
    three 2-bit steps or the special values."""
    rng = np.random.default_rng(sum(name.encode()))
    n = M4_LARGE * (e['ntrack'] // 2)
    x = rng.standard_normal(n, dtype=np.float32) * np.float32(2.2)
    pool = es.step_pool('vdif', 2, ulps=4096)
    at = rng.integers(0, n, n // 4)
    x[at] = pool[rng.integers(0, pool.size, at.size)]
    x[:es.SPECIALS.size] = es.SPECIALS
    x[16:16 + 6 * 8] = np.repeat(es.floats_at(es.oracle_steps('vdif', 2)[0][1:][:, None] + [-1, 0]).ravel(), 8)
    return x


@pytest.fixture(scope='module')
def m4_maps():
    with open(golden_path('mark4_bitmaps.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', ['2_2_4', '4_2_4', '8_2_2', '8_2_4', '16_ft_2'])
def test_mark4_encoder_matches_cpu_restatement(m4_maps, name):
    import torch
    from baseband_amd import kernels, _lib
    e = m4_maps[name]
    nt, sb, mb = e['ntrack'], e['sign_bit'], e['mag_bit']
    opw, wbytes = nt // 2, nt // 8
    x = _m4_input(name, e)
    codes = orc.encode_codes(x, 'vdif', 2)
    want = torch.from_numpy(es.mark4_encode_np(x, nt, sb, mb)).cuda()
    levels = torch.from_numpy(orc.LEVELS_2.view(np.int32)).cuda()[torch.from_numpy(codes).cuda().long()]
    xd = torch.from_numpy(x).cuda()
    u8 = C.c_uint8 * 32
    cases = [(nw, 0) for nw in _m4_word_counts(nt)] + [(M4_LARGE, cap) for cap in (0, 1, 5)]
    for direct in (0, 1):
        for nw, cap in cases:
            nb = nw * wbytes
            buf = torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
            with _knobs(direct=direct, blocks=cap):
                rc = _lib.lib.bb_encode_mark4(C.c_void_p(xd.data_ptr()), nw, nt, u8(*sb), u8(*mb),
                                              C.c_void_p(buf.data_ptr() + GUARD), nb, _stream())
                launched = _lib.last_kernel()
            assert rc == _lib.BB_OK
            assert launched.startswith('k_encode_mark4<%d,%s>' % (nt, 'direct' if direct else 'thresholds')), launched
            if cap:
                assert launched.endswith('grid %d' % cap), launched
            what = (name, direct, nw, cap)
            assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nb:] == 0xA5).all()), what
            assert torch.equal(buf[GUARD:GUARD + nb], want[:nb]), what
            # and back (the decoder reads whole 8-byte words: the guard band is its slack)
            dec = kernels.decode_mark4(buf[GUARD:], 1, nt, nw, sb, mb)
            assert torch.equal(dec.view(torch.int32), levels[:nw * opw]), what
        # the wrapper gives the same words
        with _knobs(direct=direct):
            got = kernels.encode_mark4(xd[:4097 * opw].reshape(-1, e['nchan']), nt, sb, mb)
        assert torch.equal(got, want[:4097 * wbytes]), (name, direct)


# =============================================================================
# D. device views
# =============================================================================
def _views(base):
    """(label, view) of a 1-D float32 device tensor: contiguous views that start
    1, 2, 3 elements in, a strided slice and a transposed block."""
    n = (base.numel() - 8) // 64 * 64
    out = [('[%d:]' % k, base[k:k + n]) for k in (1, 2, 3)]
    out.append(('[1::2]', base[1:1 + n][::2]))
    out.append(('[::3]', base[:n // 3 * 3][::3][:n // 3 // 32 * 32]))
    out.append(('T', base[4:4 + n].reshape(64, -1).t()))
    out.append(('[1:].T', base[1:1 + n].reshape(-1, 64).t()))
    return out


@pytest.mark.parametrize('coder,bps', CASES)
def test_encode_flat_takes_any_device_view(coder, bps):
    import torch
    from baseband_amd import kernels
    rng = np.random.default_rng(40 + bps)
    host = es.mixed_input(coder, bps, rng.standard_normal(64 * 300 + 8).astype(np.float32), seed=3)
    base = torch.from_numpy(host).cuda()
    keep = base.clone()
    assert base.data_ptr() % 16 == 0
    for label, v in _views(base):
        assert label in ('T', '[::3]') or v.data_ptr() % 16 or not v.is_contiguous()
        got = kernels.encode_flat(v, CODERS[coder], bps)
        fresh = v.clone(memory_format=torch.contiguous_format)
        assert fresh.data_ptr() % 16 == 0 and fresh.is_contiguous()
        assert torch.equal(got, kernels.encode_flat(fresh, CODERS[coder], bps)), label
        assert np.array_equal(got.cpu().numpy(), es.oracle_packed(fresh.cpu().numpy().ravel(), coder, bps)), label
    assert torch.equal(base.view(torch.int32), keep.view(torch.int32))
    # complex samples that start at an odd sample: 8 bytes into a 16-byte unit
    z = torch.view_as_complex(base[:64 * 300].reshape(-1, 2))
    for v in (z[1:1 + 4096], z[3:3 + 4096], z[1:1 + 8192:2], z[:4096].reshape(64, 64).t()):
        got = kernels.encode_flat(v, CODERS[coder], bps)
        fresh = v.clone(memory_format=torch.contiguous_format)
        assert torch.equal(got, kernels.encode_flat(fresh, CODERS[coder], bps))
        flat = torch.view_as_real(fresh).cpu().numpy().ravel()
        assert np.array_equal(got.cpu().numpy(), es.oracle_packed(flat, coder, bps))
    assert torch.equal(base.view(torch.int32), keep.view(torch.int32))


@pytest.mark.parametrize('name', ['2_2_4', '4_2_4', '8_2_4'])
def test_encode_mark4_takes_any_device_view(m4_maps, name):
    import torch
    from baseband_amd import kernels
    e = m4_maps[name]
    nt, sb, mb, nchan = e['ntrack'], e['sign_bit'], e['mag_bit'], e['nchan']
    rng = np.random.default_rng(nt)
    host = (rng.standard_normal(64 * 300 + 8) * 2.2).astype(np.float32)
    base = torch.from_numpy(host).cuda()
    keep = base.clone()
    for label, v in _views(base):
        v = v.reshape(-1, nchan) if v.is_contiguous() else v
        got = kernels.encode_mark4(v, nt, sb, mb)
        fresh = v.clone(memory_format=torch.contiguous_format)
        assert torch.equal(got, kernels.encode_mark4(fresh, nt, sb, mb)), label
        assert np.array_equal(got.cpu().numpy(), es.mark4_encode_np(fresh.cpu().numpy().ravel(), nt, sb, mb)), label
    assert torch.equal(base.view(torch.int32), keep.view(torch.int32))


def test_aligned_inputs_are_encoded_in_place(monkeypatch, m4_maps):
    """The wrappers hand the library the caller's own pointer when it can take
    it (contiguous float32 on a 16-byte boundary), and a copy's otherwise."""
    import torch
    from baseband_amd import kernels
    seen = []

    def spy(real):
        def call(d_in, *rest):
            seen.append(getattr(d_in, 'value', d_in))
            return real(d_in, *rest)
        return call
    monkeypatch.setattr(kernels.lib, 'bb_encode_flat', spy(kernels.lib.bb_encode_flat))
    monkeypatch.setattr(kernels.lib, 'bb_encode_mark4', spy(kernels.lib.bb_encode_mark4))
    base = torch.randn(4096 + 8, device='cuda')
    e = m4_maps['2_2_4']

    def encoders(v):
        kernels.encode_flat(v, 0, 2)
        kernels.encode_mark4(v.reshape(-1, 2), 16, e['sign_bit'], e['mag_bit'])
    for v in (base[:4096], base[4:4100], base[8:].reshape(-1, 2), base[:4096].reshape(2, 4, -1)):
        del seen[:]
        encoders(v)
        assert seen == [v.data_ptr(), v.data_ptr()]
    z = torch.view_as_complex(base[:4096].reshape(-1, 2))
    for v in (z, z[2:], z[6:1030]):
        del seen[:]
        kernels.encode_flat(v, 0, 2)
        assert seen == [v.data_ptr()]
    for v in (base[1:4097], base[2:4098], base[3:4099], z[1:2045], base[:4096][::2]):
        del seen[:]
        kernels.encode_flat(v, 0, 2)
        assert len(seen) == 1 and seen[0] != v.data_ptr() and seen[0] % 16 == 0


def _writer_cases(manifest, tmp_path):
    """format -> (function that opens a stream writer on given file names,
    number of files).  Small frames, and in every format a complete sample of
    4 or 8 bytes, so that dev[1:] and dev[3:] start off a 16-byte boundary."""
    from baseband_amd import gsb, mark5b, vdif, dada, guppi, mark4
    block = np.load(golden_path('block_writer_cases.npz'))
    t0 = np.datetime64('2015-06-01T01:02:03')
    m4 = manifest['m4_t16_f4']

    def block_header(mod, key, **keys):
        """A golden file's header with one polarisation and one channel."""
        cls = mod.DADAHeader if mod is dada else mod.GUPPIHeader
        header = cls.fromfile(io.BytesIO(block[key + '_file'].tobytes())).copy()
        for name, value in keys.items():
            header[name] = value
        assert int(np.prod(header.sample_shape)) == 1
        return header
    return {
        'gsb': (lambda f: gsb.open(f[0], 'ws', raw=f[1], time=t0, samples_per_frame=64, sample_rate=1e3), 2),
        'mark5b': (lambda f: mark5b.open(f[0], 'ws', sample_rate=32e6, nchan=1, bps=2,
                                         time=np.datetime64('2014-06-13T05:30:01')), 1),
        'vdif1': (lambda f: vdif.open(f[0], 'ws', sample_rate=1.6e6, nthread=1, edv=0, bps=2, nchan=1,
                                      samples_per_frame=1600, station='ab', time=t0, squeeze=False), 1),
        'vdif2': (lambda f: vdif.open(f[0], 'ws', sample_rate=1.6e6, nthread=2, edv=0, bps=2, nchan=1,
                                      samples_per_frame=1600, station='ab', time=t0, squeeze=False), 1),
        'dada': (lambda f: dada.open(f[0], 'ws', header0=block_header(dada, 'dada_real', NCHAN=1)), 1),
        'dada-complex': (lambda f: dada.open(f[0], 'ws', header0=block_header(dada, 'dada', NPOL=1)), 1),
        'guppi': (lambda f: guppi.open(f[0], 'ws', header0=block_header(guppi, 'guppi_tf', NPOL=1, OBSNCHAN=1)), 1),
        'guppi-cf': (lambda f: guppi.open(f[0], 'ws', header0=block_header(guppi, 'guppi_cf', NPOL=1, OBSNCHAN=1)), 1),
        'mark4': (lambda f: mark4.open(f[0], 'ws', sample_rate=m4['frame_rate'] * m4['samples_per_frame'],
                                       ntrack=16, fanout=4, bps=2, time=np.datetime64(m4['start_time'])), 1),
    }


@pytest.mark.parametrize('fmt', ['gsb', 'mark5b', 'vdif1', 'vdif2', 'dada', 'dada-complex', 'guppi', 'guppi-cf', 'mark4'])
@pytest.mark.parametrize('k', [1, 3])
def test_stream_writers_take_device_views(manifest, tmp_path, fmt, k):
    """fw.write(dev[k:]) -- whole frames, encoded from the caller's tensor
    itself -- writes the file fw.write(dev[k:].clone()) writes."""
    import torch
    opener, nfiles = _writer_cases(manifest, tmp_path)[fmt]
    files = {}
    for how in ('view', 'copy'):
        names = [str(tmp_path / ('%s_%s_%d' % (fmt, how, i))) for i in range(nfiles)]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with opener(names) as fw:
                spf, shape = fw.samples_per_frame, tuple(fw.sample_shape)
                g = torch.Generator(device='cuda').manual_seed(5)
                n = k + 2 * spf
                dev = torch.randn((n,) + shape + ((2,) if fw.complex_data else ()), device='cuda', generator=g) * 2.
                if fw.complex_data:
                    dev = torch.view_as_complex(dev)
                keep = dev.clone()
                v = dev[k:]
                assert v.data_ptr() == dev.data_ptr() + k * dev[0].numel() * dev.element_size()
                assert v.data_ptr() % 16, "every case is meant to be misaligned"
                fw.write(v if how == 'view' else v.clone())
                assert fw.tell() == 2 * spf
            assert torch.equal(torch.view_as_real(dev) if dev.is_complex() else dev,
                               torch.view_as_real(keep) if keep.is_complex() else keep)
        files[how] = [open(nm, 'rb').read() for nm in names]
    assert all(len(b) for b in files['view'])
    assert files['view'] == files['copy']


def test_payloads_take_device_views(manifest):
    import torch
    from baseband_amd.vdif import VDIFPayload
    from baseband_amd.mark5b import Mark5BPayload
    from baseband_amd.mark4 import Mark4Payload, Mark4Header
    from baseband_amd.dada import DADAPayload
    from baseband_amd.gsb import GSBPayload
    g = torch.Generator(device='cuda').manual_seed(9)
    dev = torch.randn(40000 + 16, device='cuda', generator=g) * 2.
    for k in (1, 3):
        v = dev[k:k + 4000]
        assert v.data_ptr() % 16
        for bps in (1, 2, 4, 8):
            a = VDIFPayload.fromdata(v.reshape(-1, 1), bps=bps)
            b = VDIFPayload.fromdata(v.clone().reshape(-1, 1), bps=bps)
            assert a == b and np.array_equal(a.words, b.words)
            want = es.oracle_packed(v.cpu().numpy(), 'vdif', bps)
            assert np.array_equal(a.words.view(np.uint8), want)
        zv = torch.view_as_complex(dev[:8000].reshape(-1, 2))[k:k + 2000].reshape(-1, 1)
        a, b = VDIFPayload.fromdata(zv, bps=2), VDIFPayload.fromdata(zv.clone(), bps=2)
        assert np.array_equal(a.words, b.words)
        a = DADAPayload.fromdata(zv.reshape(-1, 1, 1), bps=8)
        b = DADAPayload.fromdata(zv.clone().reshape(-1, 1, 1), bps=8)
        assert np.array_equal(a.words, b.words)
        a = GSBPayload.fromdata(v.reshape(-1, 1), bps=4)
        b = GSBPayload.fromdata(v.clone().reshape(-1, 1), bps=4)
        assert np.array_equal(a.words, b.words)
        assert np.array_equal(a.words.view(np.uint8), es.oracle_packed(v.cpu().numpy(), 'int', 4))
        v5 = dev[k:k + 40000]                             # (a Mark 5B payload is 10000 bytes)
        a = Mark5BPayload.fromdata(v5.reshape(-1, 1), bps=2)
        b = Mark5BPayload.fromdata(v5.clone().reshape(-1, 1), bps=2)
        assert np.array_equal(a.words, b.words)
        # item assignment: a slice, and the whole payload
        for sl in (slice(8, 8 + 1000), slice(None)):
            pa = VDIFPayload.fromdata(torch.zeros(4000, 1, device='cuda'), bps=2)
            pb = VDIFPayload.fromdata(torch.zeros(4000, 1, device='cuda'), bps=2)
            src = dev[k:k + len(range(*sl.indices(4000)))].reshape(-1, 1)
            pa[sl] = src
            pb[sl] = src.clone()
            assert np.array_equal(pa.words, pb.words) and pa.words.any()
    case = manifest['m4_t16_f4']
    h4 = Mark4Header(np.array(case['header0_words'], np.uint32), decade=2010)
    nbody = h4.samples_per_frame - 160 * h4.fanout
    body = (torch.randn((nbody + 3) * h4.nchan, device='cuda', generator=g) * 2.).reshape(-1, h4.nchan)
    for k in (1, 3):
        v = body[k:k + nbody]
        pa, pb = Mark4Payload.fromdata(v, h4), Mark4Payload.fromdata(v.clone(), h4)
        assert np.array_equal(pa.words, pb.words)
