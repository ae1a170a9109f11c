"""The frame-search kernels (k_vdif_locate, k_mark5b_locate, k_mark4_locate: bb_locate_sweep),
the header scans (k_vdif_scan, k_vdif_scan_at, k_mark5b_scan, k_mark4_scan) and the index kernels
(k_build_index, k_verify_records, k_index_verify) against the brute-force CPU restatements of
oracle/bb_index_np.py, which tests/test_index_oracle.py pins to the reference.

Every comparison is exact: sorted offsets as lists (a duplicate is a failure), all four record
fields, exact counts.  The expectation always comes from bb_index_np on ``buf[:nbytes]``, never
from the bookkeeping of the builders below and never from the kernels.

Geometry the shapes below are aimed at (k_scan.h): a lane probes 16 byte positions and takes the
dword behind them from the next lane (seam every 16 bytes), the next wave (1024), behind the
workgroup's 4 KiB chunk (4096); a workgroup takes 16 KiB per iteration (16384) and steps by the
grid; candidates are parked in a 1024-entry list per workgroup.

Left out, because the reference leaves it undefined (it raises): BCD nibbles above 9 in a Mark 5B
time code handed to the SCAN (the search does not decode them and is tested with arbitrary
nibbles).  k_index_verify has no entry point of its own: it is reached through the Mark 5B and
VDIF *_read_window calls."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import golden_path

import bb_index_np as ix

pytestmark = pytest.mark.gpu

with open(golden_path('locate_whole_cases.json')) as _f:
    WHOLE = json.load(_f)['cases']

PAD = 4096          # the device allocation is this much larger than any nbytes
FORMATS = ['vdif32', 'vdif16', 'vdif40', 'mark5b', 'mark5b_w1', 'mark4_16', 'mark4_32', 'mark4_64']


# ---- formats ---------------------------------------------------------------------------------
class Fmt:
    """One search configuration: how to write a valid header, where the sweep's probe dword
    lies in it, and the kernel / restatement pair."""

    def __init__(self, name):
        self.name = name
        self.user = 0xf00f
        if name.startswith('vdif'):
            self.kind = 'vdif'
            self.F, self.H, self.mask, self.edv = {'vdif32': (5032, 32, 'edv0', 0), 'vdif16': (1032, 16, 'legacy', 0),
                                                   'vdif40': (40, 32, 'edv3', 3),
                                                   'vdif10k': (10240, 32, 'edv0_1thread', 0),
                                                   'vdif_w2': (8200, 32, 'word2_only', 0)}[name]
            self.probe = 8
            pat = ix.vdif_header_words(self.F, self.H, seconds=100, edv=self.edv)
            self.pattern, self.maskw = pat + [0] * (8 - len(pat)), ix.VDIF_MASKS[self.mask]
        elif name.startswith('mark5b'):
            self.kind, self.F, self.H, self.probe = 'mark5b', ix.M5B_FRAME, 16, 0
            self.w1 = (self.user << 16, 0xffff0000) if name == 'mark5b_w1' else (0, 0)
        else:
            self.kind, self.ntrack = 'mark4', int(name.split('_')[1])
            self.F, self.H, self.probe = self.ntrack * 2500, self.ntrack * 20, 64 * self.ntrack // 8 - 1

    def header(self, k, rng):
        if self.kind == 'vdif':
            w = ix.vdif_header_words(self.F, self.H, seconds=int(rng.integers(0, 2 ** 30)),
                                     frame_nr=int(rng.integers(0, 2 ** 24)), edv=self.edv,
                                     thread_id=0 if self.mask == 'edv0_1thread' else int(rng.integers(0, 1024)),
                                     invalid=int(rng.integers(0, 2)))
            return ix.words_to_bytes(w)
        if self.kind == 'mark5b':
            # (any time-code bits with their CRC: the search does not decode them)
            return ix.words_to_bytes(ix.mark5b_header_words(frame_nr=k & 0x7fff, user=self.user,
                                                            frac=int(rng.integers(0, 2 ** 16)),
                                                            w2=int(rng.integers(0, 2 ** 32))))
        return ix.mark4_header_stream(self.ntrack, uyear=4, day=1 + k % 365, sec=k % 60)

    def oracle(self, buf):
        if self.kind == 'vdif':
            return ix.vdif_locate(buf, self.F, self.H, self.pattern, self.maskw).tolist()
        if self.kind == 'mark5b':
            return ix.mark5b_locate(buf, *self.w1).tolist()
        return ix.mark4_locate(buf, self.ntrack).tolist()

    def kernel(self, dbuf, nbytes):
        from baseband_amd import kernels
        if self.kind == 'vdif':
            t = kernels.vdif_locate(dbuf, nbytes, self.F, self.H, self.pattern, self.maskw)
        elif self.kind == 'mark5b':
            t = kernels.mark5b_locate(dbuf, nbytes, *self.w1)
        else:
            t = kernels.mark4_locate(dbuf, nbytes, self.ntrack)
        return t.cpu().numpy().tolist()

    def raw(self, dptr, nbytes, offs, cap, count):
        """The C entry point itself -> return code."""
        from baseband_amd import kernels
        from baseband_amd._lib import lib
        if self.kind == 'vdif':
            p = kernels._vdif_params(self.F, self.H, self.pattern, self.maskw, 0, 0, 0)
            return lib.bb_vdif_locate(dptr, nbytes, C.byref(p), kernels._ptr(offs), cap, kernels._ptr(count), None)
        if self.kind == 'mark5b':
            return lib.bb_mark5b_locate_stream(dptr, nbytes, self.w1[0], self.w1[1], kernels._ptr(offs), cap,
                                               kernels._ptr(count), None)
        return lib.bb_mark4_locate(dptr, nbytes, self.ntrack, kernels._ptr(offs), cap, kernels._ptr(count), None)

    def junk(self):
        """Four bytes that pass the sweep's probe, for repeating."""
        if self.kind == 'vdif':
            return ix.words_to_bytes([self.pattern[2]])
        if self.kind == 'mark5b':
            return ix.words_to_bytes([ix.M5B_SYNC])
        return np.array([0, 0xff, 0xff, 0xff], np.uint8)

    def damage(self, buf, pos):
        """Damage the header at pos in place, under the mask / inside the pattern."""
        if self.kind == 'vdif':
            buf[pos + 10] ^= 0x55
        elif self.kind == 'mark5b':
            buf[pos + 2] ^= 0x55
        else:
            buf[pos + 70 * self.ntrack // 8] ^= 0x10


def plant(fmt, size, starts, rng, background=None):
    """Random bytes with a valid header written at every position of `starts` (the payloads are
    whatever lies there).  Headers that would not fit are cut at the end."""
    buf = rng.integers(0, 256, size, dtype=np.uint8) if background is None else background
    for k, s in enumerate(starts):
        h = fmt.header(k, rng)[:max(0, size - s)]
        buf[s:s + len(h)] = h
    return buf


def chain(fmt, start, n, slips=()):
    """Frame starts: n frames one frame apart, `slips[i]` extra bytes in front of frame i + 1."""
    out, p = [], start
    for k in range(n):
        out.append(p)
        p += fmt.F + (slips[k] if k < len(slips) else 0)
    return out


def both_ways(fmt, full, nbytes):
    """The kernel on buf[:nbytes], once with zeros behind nbytes in the (larger) allocation and once
    with the file's continuation there: both must equal the restatement on buf[:nbytes]."""
    from baseband_amd import kernels
    want = fmt.oracle(full[:nbytes])
    zeros = np.zeros(max(len(full), nbytes) + PAD, np.uint8)
    zeros[:nbytes] = full[:nbytes]
    got_z = fmt.kernel(kernels.to_device_bytes(zeros), nbytes)
    cont = np.zeros(len(zeros), np.uint8)
    cont[:len(full)] = full
    cont[len(full):] = 0xff                      # (and no zeros behind the file either)
    got_c = fmt.kernel(kernels.to_device_bytes(cont), nbytes)
    assert got_z == want, (fmt.name, nbytes, 'zeros behind nbytes')
    assert got_c == want, (fmt.name, nbytes, 'continuation behind nbytes')
    return want


# ---- search kernels --------------------------------------------------------------------------
def _whole_fmt(c):
    if c['fmt'] == 'vdif':
        return Fmt({5032: 'vdif32', 1032: 'vdif16', 40: 'vdif40'}[c['frame_nbytes']])
    if c['fmt'] == 'mark5b':
        return Fmt('mark5b_w1' if c.get('w1_mask') else 'mark5b')
    return Fmt('mark4_%d' % c['ntrack'])


@pytest.mark.parametrize('kind', ['vdif', 'mark5b', 'mark4'])
def test_recorded_cases(kind):
    """Every buffer of locate_whole_cases.json, rebuilt from its seed, through the kernel: the list
    equals the reference's recorded answer (VDIF: combined as include/bbdecode.h states), with zeros
    and with the file's continuation behind nbytes.

    Holds the truncated-tail cases in which bb_load_u32_any used to read the top bytes of the
    following sync word as zero: Mark 5B, frame start 1 / 2 / 3 and 4-6 / 4-5 / 4 bytes of the
    following header inside the buffer."""
    from test_index_oracle import whole_case_want
    cases = [c for c in WHOLE if c['fmt'] == kind]
    assert len(cases) > 100
    failed = []
    for c in cases:
        full, nbytes = ix.build_whole_case(c)
        assert ix.sha256(full[:nbytes]) == c['sha256']
        fmt = _whole_fmt(c)
        want = whole_case_want(c)
        assert fmt.oracle(full[:nbytes]) == want
        try:
            both_ways(fmt, full, nbytes)
        except AssertionError as exc:
            failed.append((c['start'], c.get('cut'), c['damaged'], c['slips'], str(exc)[:60]))
    print(kind, 'failed:', failed)
    assert not failed


@pytest.mark.parametrize('name', FORMATS)
@pytest.mark.parametrize('blocks', [0, 3])
def test_every_position_class(name, blocks):
    """Frame starts such that the probe dword lies at all 16 residues mod 16 and straddles each seam
    of the sweep: lane 63 -> next wave (1024), the workgroup's chunk (4096), its iteration (16384),
    the grid step (3 workgroups: 49152) and a far one (65536); a slip walks the residues on."""
    from baseband_amd import kernels, _lib
    fmt = Fmt(name)
    rng = np.random.default_rng(1000 + len(name))
    kernels.tune(_lib.TUNE_BLOCKS, blocks)
    try:
        for seam in (1024, 4096, 16384, 49152, 65536):
            for d in range(-5, 12):
                start = seam + d - fmt.probe
                if start < 0:
                    continue
                starts = chain(fmt, start, 5, slips=(0, 0, 1 + d % 7))
                size = starts[-1] + fmt.F + int(rng.integers(0, 40))
                full = plant(fmt, size, starts, rng)
                want = both_ways(fmt, full, size)
                assert len(want) >= 3, (seam, d)     # (the frames in front of the slip and of the ragged end drop out)
    finally:
        kernels.tune(_lib.TUNE_BLOCKS, 0)


def _refusals(fmt):
    """(label, mutation(buf, starts), must the answer change?) -- one reason to refuse at a time, at a
    position whose probe still passes."""
    F = fmt.F
    out = []
    if fmt.kind == 'vdif':
        for k in range(fmt.H // 4):
            if fmt.maskw[k] and k != 2:
                bit = (fmt.maskw[k] & -fmt.maskw[k]).bit_length() - 1

                def mut(buf, s, k=k, bit=bit):
                    buf[s[1] + 4 * k + bit // 8] ^= 1 << bit % 8
                out.append(('word %d off under the mask' % k, mut, True))
        out.append(('next damaged in place, the one after intact', lambda buf, s: fmt.damage(buf, s[2]), True))

        def two(buf, s):
            fmt.damage(buf, s[2])
            fmt.damage(buf, s[3])
        out.append(('next two damaged', two, True))
        out.append(('last frame without a header one frame earlier', lambda buf, s: fmt.damage(buf, s[-2]), True))
    elif fmt.kind == 'mark5b':
        out.append(('CRC one bit off', lambda buf, s: buf.__setitem__(s[1] + 9, buf[s[1] + 9] ^ 4), True))
        out.append(('CRC field one bit off', lambda buf, s: buf.__setitem__(s[1] + 12, buf[s[1] + 12] ^ 1), True))
        out.append(('next sync absent', lambda buf, s: fmt.damage(buf, s[2]), True))
        out.append(('word 1 off here', lambda buf, s: buf.__setitem__(s[1] + 7, buf[s[1] + 7] ^ 0x80),
                    fmt.w1[1] != 0))
        out.append(('word 1 low half off here', lambda buf, s: buf.__setitem__(s[1] + 4, buf[s[1] + 4] ^ 1), False))
    else:
        isz = fmt.ntrack // 8
        out.append(('zero word not zero', lambda buf, s: buf.__setitem__(s[1] + 63 * isz, 0x20), True))
        if isz > 1:
            out.append(('zero word not zero in its last byte but one',
                        lambda buf, s: buf.__setitem__(s[1] + 64 * isz - 2, 1), True))
        for label, at in (('first', 64 * isz), ('fourth', 64 * isz + 3), ('middle', 80 * isz + 1),
                          ('last', 96 * isz - 1)):
            out.append(('ones run broken at its %s byte' % label,
                        lambda buf, s, at=at: buf.__setitem__(s[1] + at, 0x7f), True))
        out.append(('next pattern absent', lambda buf, s: fmt.damage(buf, s[2]), True))
        out.append(('byte behind the pattern', lambda buf, s: buf.__setitem__(s[1] + 96 * isz, 0), False))
    out.append(('last frame damaged', lambda buf, s: fmt.damage(buf, s[-1]), True))
    return out


@pytest.mark.parametrize('name', FORMATS)
def test_every_reason_to_refuse(name):
    fmt = Fmt(name)
    rng = np.random.default_rng(2000 + len(name))
    for start in (0, 7, 4090 - fmt.probe):
        if start < 0:
            continue
        starts = chain(fmt, start, 5)
        size = starts[-1] + fmt.F
        clean = plant(fmt, size, starts, rng)
        base = both_ways(fmt, clean, size)
        assert base == starts
        for label, mut, changes in _refusals(fmt):
            buf = clean.copy()
            mut(buf, starts)
            want = both_ways(fmt, buf, size)
            assert (want != base) == changes, (label, want)
    # a lone frame (nothing to check it against: it counts), and one with a stray partner two frames on
    lone = plant(fmt, fmt.F + 300, [7], rng)
    assert both_ways(fmt, lone, 7 + fmt.F) == [7]
    both_ways(fmt, lone, len(lone))                 # (with 200 bytes of something else behind it)
    far = plant(fmt, 3 * fmt.F + 50, [10, 10 + 2 * fmt.F], rng)
    both_ways(fmt, far, len(far))


@pytest.mark.parametrize('name', FORMATS)
def test_buffer_ends(name):
    """nbytes at every residue mod 16; the last frame ending exactly at nbytes and 1-3 bytes short; a
    tail of 1 .. header_nbytes + 4 bytes of a following valid header, frame starts aligned and not.
    (Mark 4 with 32 and 64 tracks: the tails within 5 bytes of a place where the answer can change.)"""
    fmt = Fmt(name)
    rng = np.random.default_rng(3000 + len(name))
    tails = list(range(-3, fmt.H + 5))
    if fmt.kind == 'mark4' and fmt.ntrack > 16:
        isz = fmt.ntrack // 8
        tails = sorted({t for c in (0, 63 * isz, 64 * isz, 96 * isz, fmt.H) for t in range(c - 5, c + 6)})
    for start in (0, 1, 2, 3, 5, 10, 15):
        starts = chain(fmt, start, 3)
        full = plant(fmt, starts[-1] + fmt.F + 64, starts, rng)
        for t in (tails if start < 4 else range(-3, 20)):
            both_ways(fmt, full, starts[-1] + t)
        for t in range(-3, 17):                         # ... and behind the last frame: no header follows
            both_ways(fmt, full, starts[-1] + fmt.F + t)
    # the tail is a header damaged in place
    starts = chain(fmt, 1, 3)
    full = plant(fmt, starts[-1] + fmt.F, starts, rng)
    fmt.damage(full, starts[-1])
    for t in (tails if fmt.kind != 'mark4' else tails[::3]):
        both_ways(fmt, full, starts[-1] + t)


@pytest.mark.parametrize('name', FORMATS)
def test_full_candidate_list(name):
    """Junk that passes the probe at every fourth byte, more than 1024 times inside one 16 KiB piece
    of one workgroup, real frames behind it in that piece: the candidates that find the list full are
    confirmed on the spot."""
    fmt = Fmt(name)
    rng = np.random.default_rng(4000 + len(name))
    for piece, phase in ((0, 0), (16384, 1), (32768, 3)):
        first = piece + 8192 + 200 + phase
        starts = chain(fmt, first, 4)
        if fmt.F < 1000:
            starts = chain(fmt, first, 100)
        inside = chain(fmt, piece + 40 + phase, 3) if fmt.F < 1000 else []     # ... and frames amid the junk
        size = max(starts) + fmt.F
        buf = rng.integers(0, 256, size, dtype=np.uint8)
        junk = np.tile(fmt.junk(), 2048)
        buf[piece + 16 + phase:piece + 16 + phase + len(junk)] = junk        # 2048 candidates in 8 KiB
        buf = plant(fmt, size, starts + inside, rng, background=buf)
        want = both_ways(fmt, buf, size)
        assert set(starts) <= set(want)


@pytest.mark.parametrize('name', ['vdif40', 'mark5b', 'mark4_16'])
def test_cap_and_count(name):
    """cap below the number found: *d_count is the full number, the first cap entries are distinct true
    positions, the entries behind cap are untouched."""
    import torch
    from baseband_amd import kernels
    fmt = Fmt(name)
    rng = np.random.default_rng(5000)
    starts = chain(fmt, 3, 40)
    size = starts[-1] + fmt.F
    buf = plant(fmt, size, starts, rng)
    want = fmt.oracle(buf)
    assert len(want) == 40
    dbuf = kernels.to_device_bytes(np.concatenate([buf, np.zeros(PAD, np.uint8)]))
    for cap in (0, 1, 7, 39, 40, 41):
        offs = torch.full((48,), -7, dtype=torch.int64, device='cuda')
        count = torch.zeros(1, dtype=torch.int64, device='cuda')
        assert fmt.raw(kernels._ptr(dbuf), size, offs, cap, count) == 0
        assert int(count.item()) == 40
        got = offs.cpu().numpy().tolist()
        n = min(cap, 40)
        assert len(set(got[:n])) == n and set(got[:n]) <= set(want)
        assert got[n:] == [-7] * (48 - n)


@pytest.mark.parametrize('name', ['vdif32', 'vdif16', 'mark5b_w1', 'mark4_32'])
def test_grid(name):
    """Any grid gives the same list, on a buffer of a few MiB so that workgroups loop."""
    from baseband_amd import kernels, _lib
    fmt = Fmt(name)
    rng = np.random.default_rng(6000 + len(name))
    size = 3 * 2 ** 20 + 1237
    starts, p = [], 11
    while p + fmt.F <= size:
        run = chain(fmt, p, int(rng.integers(2, 30)))
        starts += [s for s in run if s + fmt.F <= size]
        p = run[-1] + fmt.F + int(rng.integers(1, 5000))
    buf = plant(fmt, size, starts, rng)
    want = fmt.oracle(buf)
    assert len(want) > 10
    dbuf = kernels.to_device_bytes(np.concatenate([buf, np.zeros(PAD, np.uint8)]))
    try:
        for blocks in (0, 1, 3, 64):
            kernels.tune(_lib.TUNE_BLOCKS, blocks)
            assert fmt.kernel(dbuf, size) == want, blocks
    finally:
        kernels.tune(_lib.TUNE_BLOCKS, 0)


@pytest.mark.parametrize('name', FORMATS)
def test_small_and_odd_calls(name):
    import torch
    from baseband_amd import kernels, _lib
    fmt = Fmt(name)
    rng = np.random.default_rng(7000 + len(name))
    F = fmt.F
    full = plant(fmt, 3 * F, [0, F, 2 * F], rng)
    for nbytes in (0, 1, 15, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 3):
        both_ways(fmt, full, nbytes)
    # a 16-byte-aligned view into a larger tensor
    buf = plant(fmt, 2 * F + 77, [5, 5 + F], rng)
    big = np.concatenate([rng.integers(0, 256, 4096 + 48, dtype=np.uint8), buf, full])
    dbig = kernels.to_device_bytes(big)
    assert dbig.data_ptr() % 16 == 0
    assert fmt.kernel(dbig[4096 + 48:], len(buf)) == fmt.oracle(buf)
    # an unaligned d_buf: BB_EINVAL and nothing written
    offs = torch.full((8,), -7, dtype=torch.int64, device='cuda')
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    for shift in (1, 4, 8):
        assert fmt.raw(C.c_void_p(dbig.data_ptr() + shift), len(buf), offs, 8, count) == _lib.BB_EINVAL
    torch.cuda.synchronize()
    assert offs.cpu().tolist() == [-7] * 8 and int(count.item()) == 0


FUZZ_FORMATS = FORMATS + ['vdif10k', 'vdif_w2']


def _fuzz_buffer(fmt, seed):
    rng = np.random.default_rng([seed, len(fmt.name), fmt.F])
    # a few large buffers (up to 64 MiB), the rest small enough for fifty seeds to be cheap
    lg = {0: 26, 1: 24, 2: 22}.get(seed, int(rng.integers(15, 21)))
    size = int(2 ** lg - rng.integers(0, 4096))
    size = max(size, 3 * fmt.F + 100)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    starts, p = [], int(rng.integers(0, 64))
    budget = 4000                                       # (frames to plant: keeps the restatement's loop short)
    while p + fmt.H < size and len(starts) < budget:
        run = chain(fmt, p, int(rng.integers(1, 12)))
        starts += [s for s in run if s + fmt.H <= size]
        gap = int(rng.choice([0, 1, 2, 3, 5, 16, int(rng.integers(1, 3 * fmt.F))]))
        if len(starts) > budget // 2:
            gap += int(rng.integers(0, max(1, size // 50)))
        p = run[-1] + fmt.F + gap - int(rng.choice([0, 0, 1, 3]))
    plant(fmt, size, starts, rng, background=buf)
    for s in rng.choice(starts, max(1, len(starts) // 10)):
        if s + fmt.H <= size:
            fmt.damage(buf, int(s))
    for _ in range(int(rng.integers(0, 3))):            # runs of junk that passes the probe
        at = int(rng.integers(0, size - 9000))
        n = int(rng.integers(1, 2000))
        buf[at:at + 4 * n] = np.tile(fmt.junk(), n)
    nbytes = size - int(rng.choice([0, 0, int(rng.integers(0, fmt.H + 8)), int(rng.integers(0, fmt.F))]))
    return buf, nbytes


@pytest.mark.parametrize('name', FUZZ_FORMATS)
def test_fuzz(name):
    """Fifty seeds per search configuration: random runs of frames, slips, headers damaged in place,
    junk that passes the probe, a random end; buffers of 32 KiB to 64 MiB."""
    from baseband_amd import kernels
    fmt = Fmt(name)
    failed = []
    for seed in range(50):
        buf, nbytes = _fuzz_buffer(fmt, seed)
        want = fmt.oracle(buf[:nbytes])
        got = fmt.kernel(kernels.to_device_bytes(buf), nbytes)      # (the rest of the buffer lies behind nbytes)
        if got != want:
            failed.append((seed, nbytes, len(want), len(got), sorted(set(want) ^ set(got))[:5]))
    print(name, 'failed seeds:', failed)
    assert not failed


# ---- scan kernels, record for record ---------------------------------------------------------
def _same_records(got_t, want):
    from baseband_amd import kernels
    got = kernels.recs_fields(got_t)
    for key in ('payload_offset', 'time_index', 'thread_id', 'flags'):
        assert got[key].tolist() == want[key].tolist(), key


def _vdif_scan(dbuf, nbytes, where, F, H, pattern, mask, ref_s, ref_f, rate, set_n=0):
    import torch
    from baseband_amd import kernels
    if isinstance(where, tuple):
        return kernels.vdif_scan(dbuf[:nbytes], where[1], F, H, pattern, mask, ref_s, ref_f, rate,
                                 first_offset=where[0], set_nframes=set_n)
    at = torch.tensor(where, dtype=torch.int64, device='cuda')
    return kernels.vdif_scan_at(dbuf, nbytes, at, F, H, pattern, mask, ref_s, ref_f, rate)


@pytest.mark.parametrize('H,maskname', [(32, 'edv0'), (16, 'legacy'), (32, 'edv3')])
def test_vdif_scan_records(H, maskname):
    """Fixed stride and scan_at: fields over their full ranges, references far enough away for both
    clamps, frame_rate = 0, the set_nframes rule, a mismatch in each header word, the last header /
    frame cut by the buffer end; scan_at at all four byte residues and at the end of the buffer."""
    from baseband_amd import kernels
    rng = np.random.default_rng(8000 + H)
    F, n = 1032, 64
    edv = 3 if maskname == 'edv3' else 0
    mask = ix.VDIF_MASKS[maskname]
    pat = ix.vdif_header_words(F, H, edv=edv)
    pat += [0] * (8 - len(pat))
    for first in (0, 4, 1, 2, 3):
        buf = rng.integers(0, 256, first + n * F, dtype=np.uint8)
        for k in range(n):
            sec = [0, 2 ** 30 - 1, 5, 5, 6][k] if k < 5 else int(rng.integers(0, 2 ** 30))
            fnr = [0, 2 ** 24 - 1, 7, 7, 7][k] if k < 5 else int(rng.integers(0, 2 ** 24))
            if 16 <= k < 32:                                     # sets of four: equal frame numbers, other seconds
                fnr, sec = 1000 + (k // 4), 77 + k % 3
            thread = [0, 1023][k] if k < 2 else int(rng.integers(0, 1024))
            w = ix.vdif_header_words(F, H, seconds=sec, frame_nr=fnr, thread_id=thread, edv=edv,
                                     invalid=int(rng.integers(0, 2)))
            buf[first + k * F:first + k * F + H] = ix.words_to_bytes(w)
        for k in range(H // 4):                                  # a mismatch in each header word under the mask
            if mask[k]:
                bit = (mask[k] & -mask[k]).bit_length() - 1
                buf[first + (40 + k) * F + 4 * k + bit // 8] ^= 1 << bit % 8
        dbuf = kernels.to_device_bytes(np.concatenate([buf, np.full(PAD, 0xab, np.uint8)]))
        offs = [first + k * F for k in range(n)]
        ends = [len(buf), len(buf) - 1, len(buf) - F + H, len(buf) - F + H - 1, len(buf) - F + 9, len(buf) - F + 4,
                len(buf) - F]
        for ref_s, ref_f, rate, set_n in ((5, 7, 1600, 0), (0, 0, 0, 0), (2 ** 30 - 1, 0, 2 ** 20, 0),
                                          (0, 2 ** 24 - 1, 2 ** 20, 0), (77, 1000, 25000, 4), (77, 1000, 25000, 3)):
            for nbytes in ends:
                args = (F, H, pat, mask, ref_s, ref_f, rate)
                want_at = ix.vdif_records(buf[:nbytes], offs, *args)
                _same_records(_vdif_scan(dbuf, nbytes, offs, *args), want_at)
                if first % 4 == 0:
                    want = ix.vdif_records(buf[:nbytes], (first, n), *args, set_nframes=set_n)
                    _same_records(_vdif_scan(dbuf, nbytes, (first, n), *args, set_n=set_n), want)
                    if set_n == 0:                               # scan_at equals the fixed stride's records
                        for key in want:
                            assert want[key].tolist() == want_at[key].tolist()
        # offsets anywhere, also where no header is, at and behind the end
        odd = [0, 1, 2, 3, first + F + 1, len(buf) - H, len(buf) - H + 1, len(buf) - 3, len(buf), len(buf) + 40]
        args = (F, H, pat, mask, 5, 7, 1600)
        _same_records(_vdif_scan(dbuf, len(buf), odd, *args), ix.vdif_records(buf, odd, *args))


def _m5b_scan(dbuf, nbytes, where, ref_s, ref_f, rate, by_pos):
    import torch
    from baseband_amd import kernels, _lib
    p = _lib.Mark5BScanParams()
    p.ref_seconds, p.ref_frame_nr, p.frame_rate, p.by_position = ref_s, ref_f, rate, by_pos
    if isinstance(where, tuple):
        p.first_offset, n = where
        recs = torch.empty((n, 4), dtype=torch.int32, device='cuda')
        rc = _lib.lib.bb_mark5b_scan(kernels._ptr(dbuf), nbytes, C.byref(p), kernels._ptr(recs), n, None)
    else:
        at = torch.tensor(where, dtype=torch.int64, device='cuda')
        recs = torch.empty((len(where), 4), dtype=torch.int32, device='cuda')
        rc = _lib.lib.bb_mark5b_scan_at(kernels._ptr(dbuf), nbytes, C.byref(p), kernels._ptr(at), len(where),
                                        kernels._ptr(recs), None)
    assert rc == 0
    return recs


def test_mark5b_scan_records():
    """Day wrap in both directions, by_position, wrong sync, truncated frame, odd offsets; fill-pattern
    validity with a payload that is all fill, and all fill except one word at index 0, 63, 64, 2495,
    2496 and 2499.  Time codes are decimal BCD throughout: the reference raises on other nibbles
    (base/utils.py:18-40), what the scan gives for them is not defined and not tested."""
    from baseband_amd import kernels
    rng = np.random.default_rng(8100)
    F = ix.M5B_FRAME
    days = [(999, 86399), (0, 0), (0, 1), (500, 0), (499, 86399), (998, 5), (123, 45678)]
    holes = [None, 0, 63, 64, 2495, 2496, 2499]
    n = len(days) + len(holes) + 3
    for first in (0, 4, 1, 2, 3):
        buf = rng.integers(0, 256, first + n * F, dtype=np.uint8)
        for k in range(n):
            jday, sec = days[k] if k < len(days) else (123, 45678 + k)
            w = ix.mark5b_header_words(frame_nr=int(rng.integers(0, 2 ** 15)), jday=jday, seconds=sec,
                                       user=int(rng.integers(0, 2 ** 16)), frac=int(rng.integers(0, 2 ** 16)))
            at = first + k * F
            buf[at:at + 16] = ix.words_to_bytes(w)
            if len(days) <= k < len(days) + len(holes):
                buf[at + 16:at + F] = np.tile(ix.words_to_bytes([ix.M5B_FILL]), 2500)
                hole = holes[k - len(days)]
                if hole is not None:
                    buf[at + 16 + 4 * hole + int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
        buf[first + (n - 2) * F + 1] ^= 0x40                     # wrong sync
        dbuf = kernels.to_device_bytes(np.concatenate([buf, np.full(PAD, 0x44, np.uint8)]))
        offs = [first + k * F for k in range(n)]
        for ref in ((999, 86399), (0, 0), (123, 45678), (600, 0)):
            ref_s = ref[0] * 86400 + ref[1]
            for rate, by_pos in ((6400, 0), (25600, 0), (0, 0), (6400, 1), (1, 0)):
                for nbytes in (len(buf), len(buf) - 1, len(buf) - F + 16, len(buf) - F):
                    args = (ref_s, 3, rate, by_pos)
                    want_at = ix.mark5b_records(buf[:nbytes], offs, *args)
                    _same_records(_m5b_scan(dbuf, nbytes, offs, *args), want_at)
                    if first % 4 == 0:
                        want = ix.mark5b_records(buf[:nbytes], (first, n), *args)
                        _same_records(_m5b_scan(dbuf, nbytes, (first, n), *args), want)
                        for key in want:
                            assert want[key].tolist() == want_at[key].tolist()
        odd = [first + 1, first + F + 2, first + 2 * F + 3, len(buf) - F, len(buf) - F + 1, len(buf)]
        _same_records(_m5b_scan(dbuf, len(buf), odd, 0, 0, 6400, 0), ix.mark5b_records(buf, odd, 0, 0, 6400, 0))


def _m4_scan(dbuf, nbytes, where, ntrack, ref_year, ref_qms, frame_qms, by_pos):
    import torch
    from baseband_amd import kernels, _lib
    p = _lib.Mark4ScanParams()
    p.ntrack, p.ref_year, p.ref_qms, p.frame_qms, p.by_position = ntrack, ref_year, ref_qms, frame_qms, by_pos
    if isinstance(where, tuple):
        p.first_offset, n = where
        recs = torch.empty((n, 4), dtype=torch.int32, device='cuda')
        rc = _lib.lib.bb_mark4_scan(kernels._ptr(dbuf), nbytes, C.byref(p), kernels._ptr(recs), n, None)
    else:
        at = torch.tensor(where, dtype=torch.int64, device='cuda')
        recs = torch.empty((len(where), 4), dtype=torch.int32, device='cuda')
        rc = _lib.lib.bb_mark4_scan_at(kernels._ptr(dbuf), nbytes, C.byref(p), kernels._ptr(at), len(where),
                                       kernels._ptr(recs), None)
    assert rc == 0
    return recs


@pytest.mark.parametrize('ntrack', [16, 32, 64])
def test_mark4_scan_records(ntrack):
    """Times on and off the frame grid, decade roll-over into a leap and a non-leap year, a foreign
    decade digit, each of the four error-flag words, sync broken at word 63 and at the first, a middle
    and the last of words 64-95, a nibble above 9 in each BCD field (counted as include/bbdecode.h
    says; the record is not OK), by_position, unaligned offsets."""
    from baseband_amd import kernels
    rng = np.random.default_rng(8200 + ntrack)
    isz, F = ntrack // 8, ntrack * 2500
    heads = [dict(uyear=5, day=1, ms=0), dict(uyear=5, day=1, ms=5), dict(uyear=5, day=1, ms=3),
             dict(uyear=5, day=365, hour=23, minute=59, sec=59, ms=995), dict(uyear=6, day=1),
             dict(uyear=6, day=2, ms=125), dict(uyear=7, day=1), dict(uyear=4, day=366),
             dict(uyear=5, day=100, flags=8), dict(uyear=5, day=100, flags=4), dict(uyear=5, day=100, flags=2),
             dict(uyear=5, day=100, flags=1), dict(uyear=5, day=200, sec=30),
             dict(uyear=5, bcd=(5 << 28 | 0x1a0 << 16, 0)), dict(uyear=5, bcd=(5 << 28 | 0x001 << 16 | 0x2b << 8, 0)),
             dict(uyear=5, bcd=(5 << 28 | 0x001 << 16 | 0x6c, 0)), dict(uyear=5, bcd=(5 << 28 | 0x001 << 16, 0x0d << 12)),
             dict(uyear=5, bcd=(5 << 28 | 0x001 << 16, 0x0e0)), dict(uyear=5, bcd=(5 << 28 | 0x001 << 16, 0x00f))]
    breaks = [63 * isz, 64 * isz - 1, 64 * isz, 80 * isz + isz // 2, 96 * isz - 1]
    n = len(heads) + len(breaks)
    for first in (0, isz, 1, 3):
        buf = rng.integers(0, 256, first + n * F, dtype=np.uint8)
        for k in range(n):
            at = first + k * F
            buf[at:at + 20 * ntrack] = ix.mark4_header_stream(ntrack, **(heads[k] if k < len(heads)
                                                                       else dict(uyear=5, day=1 + k)))
            if k >= len(heads):
                buf[at + breaks[k - len(heads)]] ^= 0x08
        dbuf = kernels.to_device_bytes(np.concatenate([buf, np.full(PAD, 0xff, np.uint8)]))
        offs = [first + k * F for k in range(n)]
        for ref_year, ref_qms, frame_qms, by_pos in ((2015, 0, 10, 0), (2015, 86400 * 4000, 5, 0),
                                                      (2016, 0, 10, 0), (2015, 364 * 86400 * 4000, 640, 0),
                                                      (2015, 0, 0, 0), (2015, 0, 10, 1), (2025, 4000, 20, 0),
                                                      (2015, 365 * 86400 * 4000, 10, 0),
                                                      (2016, 366 * 86400 * 4000, 10, 0)):
            for nbytes in (len(buf), len(buf) - 1, len(buf) - F):
                args = (ntrack, ref_year, ref_qms, frame_qms, by_pos)
                want_at = ix.mark4_records(buf[:nbytes], offs, *args)
                _same_records(_m4_scan(dbuf, nbytes, offs, *args), want_at)
                if first % isz == 0:
                    want = ix.mark4_records(buf[:nbytes], (first, n), *args)
                    _same_records(_m4_scan(dbuf, nbytes, (first, n), *args), want)
                    for key in want:
                        assert want[key].tolist() == want_at[key].tolist()
    # what the cases are there for does happen
    want = ix.mark4_records(buf, offs, ntrack, 2015, 0, 10, 0)
    ok = (want['flags'] & 1).tolist()
    assert ok[:8] == [1, 1, 0, 1, 1, 1, 0, 0] and ok[13:19] == [0] * 6 and ok[19:] == [0] * len(breaks)
    assert (want['flags'] >> 1).tolist()[8:12] == [1, 1, 1, 1]
    # day 1 of the year after a non-leap / a leap ref_year, counted from the end of ref_year
    assert ix.mark4_records(buf, offs, ntrack, 2015, 365 * 86400 * 4000, 10, 0)['time_index'][4] == 86400 * 400
    assert ix.mark4_records(buf, offs, ntrack, 2016, 366 * 86400 * 4000, 10, 0)['time_index'][6] == 86400 * 400


# ---- index kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(8))
def test_build_index_and_verify_records(seed):
    """Random record tables: time indices below 0 and beyond nframes_out, slots -1 and beyond nslot,
    invalid and not-OK flags, nstrict and recs_per_index varied.  No two records that are put claim the
    same slot -- that is a race by design (the last writer wins, whichever it is): the builder gives
    every record a (time index, thread) of its own."""
    import torch
    from baseband_amd import kernels
    rng = np.random.default_rng(9000 + seed)
    nslot = int(rng.choice([1, 2, 8]))
    nframes_out = int(rng.choice([1, 5, 300, 5000]))
    nthread = nslot + 2
    pairs = rng.permutation((nframes_out + 6) * nthread)[:int(rng.integers(1, 3000))]
    n = len(pairs)
    tidx = (pairs // nthread - 3).astype(np.int32)                  # -3 .. nframes_out + 2
    threads = rng.permutation(1024)[:nthread]
    slot = np.full(1024, -1, np.int16)
    for s, t in enumerate(threads):
        slot[t] = s - 1 if s <= nslot else nslot + 3                # one thread maps to -1, one beyond nslot
    recs = dict(payload_offset=rng.integers(0, 2 ** 40, n).astype(np.int64), time_index=tidx,
                thread_id=threads[pairs % nthread].astype(np.int16),
                flags=rng.choice([1, 1, 1, 0, 2, 3], n).astype(np.uint16))
    drecs = torch.from_numpy(ix.pack_recs(recs)).cuda()
    dslot = torch.from_numpy(slot).cuda()
    got = kernels.build_index(drecs, nframes_out, nslot, dslot).cpu().numpy()
    assert got.tolist() == ix.build_index(recs, nframes_out, nslot, slot).tolist()
    if nslot == 1:
        keep = np.unique(tidx, return_index=True)[1]                # (no thread map: one record per index)
        sub = {k: v[np.sort(keep)] for k, v in recs.items()}
        got = kernels.build_index(torch.from_numpy(ix.pack_recs(sub)).cuda(), nframes_out).cpu().numpy()
        assert got.tolist() == ix.build_index(sub, nframes_out, 1, None).tolist()
    # verification: records in order, some out of place
    for rpi in (1, nslot, 3):
        first = int(rng.integers(-5, 1000))
        seq = dict(recs)
        seq['time_index'] = (first + np.arange(n) // rpi).astype(np.int32)
        wrong = rng.random(n) < 0.05
        seq['time_index'][wrong] += rng.choice([-1, 1, 100], int(wrong.sum())).astype(np.int32)
        dseq = torch.from_numpy(ix.pack_recs(seq)).cuda()
        for nstrict in (0, 1, n // 2, n, n + 10):
            nbad = torch.full((1,), 5, dtype=torch.int32, device='cuda')     # the count is ADDED
            kernels.verify_records(dseq, n, first, rpi, nstrict, nbad)
            assert int(nbad.item()) == 5 + ix.verify_count(seq, first, rpi, nstrict), (rpi, nstrict)


def test_index_verify_in_one_launch():
    """k_index_verify (index and verification in one launch: only the *_read_window calls reach it)
    leaves the records, the index and the count that the restatements -- and the two separate calls --
    give.  Frames that are put have a (time index, slot) of their own; the out-of-place ones land
    outside the index."""
    import torch
    from baseband_amd import kernels, _lib
    rng = np.random.default_rng(9100)
    # Mark 5B: 20 frames and the look-ahead header
    F, n = ix.M5B_FRAME, 20
    buf = rng.integers(0, 256, (n + 1) * F, dtype=np.uint8)
    for k in range(n + 1):
        fnr = {5: 45, 11: 3000}.get(k, k)                       # two out of place (beyond the index)
        buf[k * F:k * F + 16] = ix.words_to_bytes(ix.mark5b_header_words(frame_nr=fnr, jday=321, seconds=777))
    buf[7 * F + 16:8 * F] = np.tile(ix.words_to_bytes([ix.M5B_FILL]), 2500)      # invalid
    buf[9 * F + 3] ^= 1                                          # no sync word
    dbuf = kernels.to_device_bytes(buf)
    for nstrict in (0, 6, n, n + 1):
        win = kernels.Mark5BWindow(321 * 86400 + 777, 6400, 2, 1, 0.)
        out = torch.empty(n * 40000, dtype=torch.float32, device='cuda')
        nbad = torch.full((1,), 3, dtype=torch.int32, device='cuda')
        win.run(dbuf, 0, n + 1, n, None, out, nstrict, nbad, None)
        want = ix.mark5b_records(buf, (0, n + 1), 321 * 86400 + 777, 0, 6400)
        _same_records(win.recs[:n + 1], want)
        assert win.src[:n].cpu().tolist() == ix.build_index(want, n).tolist()
        assert win.src[:n].cpu().tolist() == kernels.build_index(win.recs[:n + 1], n).cpu().tolist()
        assert int(nbad.item()) == 3 + ix.verify_count(want, 0, 1, nstrict)
        sep = torch.zeros(1, dtype=torch.int32, device='cuda')
        kernels.verify_records(win.recs[:n + 1], n + 1, 0, 1, nstrict, sep)
        assert int(sep.item()) == int(nbad.item()) - 3
    assert ix.verify_count(want, 0, 1, n) == 3 and (ix.build_index(want, n) < 0).sum() == 4

    # VDIF: 12 sets of 4 threads in file order and one more set behind them; threads through a map
    Fv, H, nsets, nth = 1032, 32, 12, 4
    mask = ix.VDIF_MASKS['edv0']
    pat = ix.vdif_header_words(Fv, H, seconds=100)
    nfr = (nsets + 1) * nth
    buf = rng.integers(0, 256, nfr * Fv, dtype=np.uint8)
    threads = [9, 1020, 0, 513]
    for k in range(nfr):
        s, t = divmod(k, nth)
        fnr = {(3, 2): 40, (11, 0): 16, (6, 1): 2 ** 24 - 1}.get((s, t), s)       # out of place: beyond the index
        thread = 77 if (s, t) == (4, 3) else threads[t]                             # a thread that is not selected
        buf[k * Fv:k * Fv + H] = ix.words_to_bytes(ix.vdif_header_words(
            Fv, H, seconds=100 + (t if s == 8 else 0), frame_nr=fnr, thread_id=thread,
            invalid=int((s, t) == (2, 2))))
    buf[(5 * nth + 1) * Fv + 10] ^= 0x20                         # a header that is none
    slot = np.full(1024, -1, np.int16)
    for i, t in enumerate(threads):
        slot[t] = [2, 0, 3, 1][i]
    dslot = torch.from_numpy(slot).cuda()
    dbuf = kernels.to_device_bytes(buf)
    for nstrict in (0, nsets * nth, nfr):
        win = kernels.VDIFWindow(Fv, H, pat, mask, 100, 1600, Fv - H, _lib.CODER_VDIF, 2, 1, nth, False, 0.)
        out = torch.empty(nsets * nth * 4000, dtype=torch.float32, device='cuda')
        nbad = torch.zeros(1, dtype=torch.int32, device='cuda')
        win.run(dbuf, 0, nfr, dslot, nsets, None, out, nth, nstrict, nbad, None)
        want = ix.vdif_records(buf, (0, nfr), Fv, H, pat, mask, 100, 0, 1600, set_nframes=nth)
        _same_records(win.recs[:nfr], want)
        want_src = ix.build_index(want, nsets, nth, slot).tolist()
        assert win.src[:nsets * nth].cpu().tolist() == want_src
        assert kernels.build_index(win.recs[:nfr], nsets, nth, dslot).cpu().tolist() == want_src
        assert int(nbad.item()) == ix.verify_count(want, 0, nth, nstrict)
    # set 8's threads carry other seconds and are placed by the set's first header all the same
    assert want['time_index'][8 * nth:9 * nth].tolist() == [8] * nth
    # (bad: three frames out of place and the header that is none; not put: those, the thread that is
    # not selected and the invalid frame)
    assert ix.verify_count(want, 0, nth, nfr) == 4 and want_src.count(-1) == 6
